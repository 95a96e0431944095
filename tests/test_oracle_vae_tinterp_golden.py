"""CPU: the oracle's t_ops decode with interp_mode "trilinear" (oracle/vae_enc_ref.decode_tile_tops) and the restatement of the two
spatial tile loops with a t_ops tile coder (tests/tops_tiled_ref.py) against tests/golden/vae_tinterp.npz, which the reference's own
code produced (tools/make_golden_vae_tinterp.py).  fp32 oracle vs fp32 reference: 1e-4, as the other golden tests.  The fp16-emulated
contract, which the GPU tests compare the kernels with, must sit within 1e-2 of the golden on these inputs: half of the 2e-2 that
tests/test_gpu_vae_tops_modes.py asserts between the kernels and the golden."""
import json

import pytest
import torch

from hunyuanvideo_efficiency_amd import synthetic as syn
from oracle import vae_enc_ref as E
from oracle import vae_ref as R
from tests import tops_tiled_ref as TR


def close(a, b, tol=1e-4):
    assert a.shape == b.shape, (a.shape, b.shape)
    err = float((a - b).abs().max() / b.abs().max())
    assert err < tol, err
    return err


def _json(t):
    return json.loads(bytes(t.numpy().tobytes()).decode())


@pytest.fixture(scope="module")
def fx(golden):
    g = golden("vae_tinterp")
    boc = tuple(g["block_out_channels"].tolist())
    sd = syn.synth_vae_state_dict(boc, seed=0, encoder=True)
    sd16 = {k: v.half().float() for k, v in sd.items()}
    ss, sl = g["tile"].tolist()
    tp = R.TileParams(sample_size=ss, n_blocks=4)
    assert tp.tile_latent_min_size == sl
    return g, boc, sd, sd16, tp


def test_fixture_holds_data_only_and_fp16_valued_inputs(fx):
    g = fx[0]
    assert set(g) == {"z", "y", "t_ops_json", "x_tiled", "moments_tiled", "z_tiled", "y_tiled", "t_ops_tiled_json", "tile", "block_out_channels"}
    for k in ("z", "x_tiled", "z_tiled"):
        assert torch.equal(g[k].half().float(), g[k]), k
    modes = {bc["interp_mode"] for bc in _json(g["t_ops_json"])["decoder"]["up_blocks"]}
    assert modes == {"trilinear"}
    # 2 x 2 tiles with a ragged last row and column, on both halves
    ss, sl = g["tile"].tolist()
    for t, size in ((g["x_tiled"], ss), (g["z_tiled"], sl)):
        ov = int(size * 0.75)
        for n in t.shape[-2:]:
            starts = list(range(0, n, ov))
            assert len(starts) == 2 and 0 < n - starts[-1] < size


def test_trilinear_decode(fx):
    g, boc, sd, sd16, _ = fx
    t_ops = _json(g["t_ops_json"])
    with torch.no_grad():
        close(E.decode_tile_tops(sd, g["z"], boc, R.FP32, t_ops), g["y"])
        close(E.decode_tile_tops(sd16, g["z"], boc, R.Prec(True), t_ops), g["y"], 1e-2)
        # the mode matters on this fixture: nearest is far from it
        near = json.loads(json.dumps(t_ops))
        for bc in near["decoder"]["up_blocks"]:
            bc["interp_mode"] = "nearest"
        y = E.decode_tile_tops(sd, g["z"], boc, R.FP32, near)
        assert float((y - g["y"]).abs().max() / g["y"].abs().max()) > 5e-2


def test_spatial_tile_loops_under_t_ops(fx):
    g, boc, sd, sd16, tp = fx
    t_ops = _json(g["t_ops_tiled_json"])
    with torch.no_grad():
        close(TR.spatial_tiled_encode(sd, g["x_tiled"], boc, tp, R.FP32, t_ops), g["moments_tiled"])
        close(TR.spatial_tiled_decode(sd, g["z_tiled"], boc, tp, R.FP32, t_ops), g["y_tiled"])
        close(TR.spatial_tiled_encode(sd16, g["x_tiled"], boc, tp, R.Prec(True), t_ops), g["moments_tiled"], 1e-2)
        close(TR.spatial_tiled_decode(sd16, g["z_tiled"], boc, tp, R.Prec(True), t_ops), g["y_tiled"], 1e-2)
        # without t_ops the restatement is the oracle's own loop
        x = g["x_tiled"][:, :, :3]
        assert torch.equal(TR.spatial_tiled_encode(sd, x, boc, tp, R.FP32), E.spatial_tiled_encode(sd, x, boc, tp, R.FP32))
        z = g["z_tiled"][:, :, :1]
        assert torch.equal(TR.spatial_tiled_decode(sd, z, boc, tp, R.FP32), R.spatial_tiled_decode(sd, z, boc, tp, R.FP32))
