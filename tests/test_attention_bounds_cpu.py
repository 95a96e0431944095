"""CPU: the attention bound of tests/attention_bounds.py has teeth.  A faithful emulation of the kernel's arithmetic - q' rounded once,
fp32 scores with the running maximum subtracted, a maximum that moves only when a tile exceeds it by more than 8 (per 32-row query
block, rescaling O and l), P rounded to bf16 for P.V, unrounded row sums, fp32 accumulation, 64-key tiles taken in any order, a
two-way KV split merged with 2^(m_s - m) - must be accepted on every data class; each way the loop can be subtly wrong must be
rejected on the data class named here:

    one 64-key tile dropped                      random (O), flat (O, and l = n_kv - 64 through m + log2 l)
    tile t replaced by tile t - 4 (stale ring)   random, peaked (the peak's tile is the stale one)
    key n_kv included as a zero row              phantom (the zero key owns the row), flat (l = n_kv + 1 through m + log2 l)
    rescale not applied to one query block's O   peaked (rows whose peak comes late)
    merge weights e^(m_s - m)                    random (the halves' maxima differ by O(1))
    q used unrounded                             random, through m + log2 l (see below)

What a data class can NOT catch (recorded, nothing loosened for it): `flat` and `phantom` give nearly uniform weights, so the
unrounded q (q = 0 is exact; a common shift of every score cancels) and the e^ merge on `flat` (both halves have m = 0) are invisible
there; on `peaked` the e^ merge only changes weights that are ~2^-18 either way.  The unrounded q moves O by less than the P-term
on every class (the score errors of ~100 effective keys average out) - it is the (m, l) check that rejects it, by ~30x its tolerance.

The P-term decision of attention_bounds.py is made here: test_p_term_form_decided_on_the_emulation measures the faithful emulation
against both forms."""
import math

import pytest
import torch

from tests import attention_bounds as AB

D, KVT, THR = AB.D, AB.KVT, AB.THR
N_Q, H = 96, 1
N_KV = 64 * 11 + 33          # 12 tiles, ragged last tile: enough tiles for a stale t - 4; ~100 effective keys on `random`


def emulate(q, k, v, order=None, drop=None, stale=None, phantom=False, skip_rescale=None, unrounded_q=False):
    """one head, one pass over the keys -> (part_o [n_q, 128] fp32, m, l).  order: permutation of the tile indices."""
    n_q, n_kv = q.shape[0], k.shape[0]
    qp = q.float() * AB.scale_log2e() if unrounded_q else AB.q_prime(q).float()
    kf, vf = k.float(), v.float()
    ntiles = (n_kv + KVT - 1) // KVT
    O = torch.zeros(n_q, D)
    l = torch.zeros(n_q)
    m = None
    for t in (order if order is not None else range(ntiles)):
        if t == drop:
            continue
        j0, j1 = t * KVT, min(n_kv, (t + 1) * KVT)
        src = j0 - 4 * KVT if t == stale else j0
        kt, vt = kf[src:src + (j1 - j0)], vf[src:src + (j1 - j0)]
        if phantom and t == ntiles - 1 and j1 - j0 < KVT:
            kt, vt = torch.cat([kt, torch.zeros(1, D)]), torch.cat([vt, torch.zeros(1, D)])
        s = qp @ kt.T
        if m is None:
            m = s.max(dim=1).values.clone()          # tile 0 fixes the initial maximum exactly
        s = s - m[:, None]
        mx = s.max(dim=1).values
        for b in range(0, n_q, 32):
            if bool((mx[b:b + 32] > THR).any()):
                d = mx[b:b + 32].clamp(min=0.0)
                alpha = torch.exp2(-d)
                l[b:b + 32] *= alpha
                m[b:b + 32] += d
                s[b:b + 32] -= d[:, None]
                if skip_rescale != b // 32:
                    O[b:b + 32] *= alpha[:, None]
        p = torch.exp2(s)
        l += p.sum(dim=1)
        O += p.to(AB.BF16).float() @ vt
    return O, m, l


def normalise(O, l):
    return (O / l[:, None]).to(AB.BF16)


def merge(parts, base_e=False):
    """attn_combine_kernel in fp32; base_e: the mutant with e^(m_s - m)"""
    m = torch.stack([p[1] for p in parts]).max(dim=0).values
    acc, l = torch.zeros_like(parts[0][0]), torch.zeros_like(m)
    for o_s, m_s, l_s in parts:
        w = torch.exp(m_s - m) if base_e else torch.exp2(m_s - m)
        acc += o_s * w[:, None]
        l += l_s * w
    return normalise(acc, l)


_CASES = {}


def case(cls, p_form="worst"):
    if (cls, p_form) not in _CASES:
        q, k, v = AB.make_case(cls, N_Q, N_KV, H, "cpu")
        _CASES[cls, p_form] = (q, k, v, AB.AttnRef(q, k, v, H, p_form=p_form))
    return _CASES[cls, p_form]


def ml(m, l):
    return torch.stack([m, l], -1)[:, None]


def accepted(ref, part):
    """the normalised output and the partials both pass -> the worst O ratio; AssertionError otherwise"""
    O, m, l = part
    r = ref.check_o(normalise(O, l), "O")
    ref.check_partial(O[:, None], ml(m, l), "partial")
    return r


def rejected(ref, part):
    with pytest.raises(AssertionError):
        accepted(ref, part)


@pytest.mark.parametrize("cls", AB.CLASSES)
def test_faithful_emulation_is_accepted(cls):
    q, k, v, ref = case(cls)
    ntiles = (N_KV + KVT - 1) // KVT
    orders = [None, list(reversed(range(ntiles))), torch.randperm(ntiles, generator=torch.Generator().manual_seed(1)).tolist()]
    for order in orders:
        r = accepted(ref, emulate(q, k, v, order=order))
        assert r <= 1.0
    # two-way KV split as hv_attn_fwd_bf16 cuts it, merged with 2^(m_s - m): within the single-pass bound (the gap covers the halves' maxima)
    cut = ((ntiles + 1) // 2) * KVT
    parts = [emulate(q, k[:cut], v[:cut]), emulate(q, k[cut:], v[cut:])]
    halves_m = torch.stack([p[1] for p in parts])
    gap = (ref.M[:, 0] - halves_m.double().min(dim=0).values).clamp(min=0.0) + THR
    AB.AttnRef(q, k, v, H, gap=gap[:, None]).check_o(merge(parts), "split")


def test_p_term_form_decided_on_the_emulation(capsys):
    """the worst-case P-term is kept: the faithful emulation uses 0.3-0.4 of the bound with it (between the 0.05 floor of the GPU ratio
    report and 1) and the output check ALONE - all the normalised entry point offers - rejects a dropped and a stale tile"""
    rows = []
    for cls in AB.CLASSES:
        q, k, v = case(cls)[:3]
        O, m, l = emulate(q, k, v)
        for form in ("worst", "stat"):
            ref = case(cls, form)[3]
            rows.append((cls, form, float(ref.ratio_o(normalise(O, l)).max()), float(ref.ratio_o(O[:, None] / l[:, None, None], final=False).max())))
    q, k, v, ref = case("random")
    mut = {"dropped tile 5": emulate(q, k, v, drop=5), "dropped tile 11 (33 keys)": emulate(q, k, v, drop=11), "stale tile 4": emulate(q, k, v, stale=4),
           "unrounded q": emulate(q, k, v, unrounded_q=True)}
    mr = {name: float(ref.ratio_o(normalise(O, l)).max()) for name, (O, m, l) in mut.items()}
    with capsys.disabled():
        print("\nfaithful emulation: largest error / bound   class    P-term   O (bf16)   part_o / l")
        for r in rows:
            print(f"                                            {r[0]:<8} {r[1]:<6} {r[2]:9.3f} {r[3]:9.3f}")
        print("mutants on `random`, O alone, worst-case form: " + ", ".join(f"{n} {x:.3g}" for n, x in mr.items()))
    by = {(r[0], r[1]): r for r in rows}
    for cls in ("random", "peaked", "phantom"):
        assert 0.05 < by[cls, "worst"][2] <= 1.0, by[cls, "worst"]
    for cls in ("random", "phantom"):
        assert 0.05 < by[cls, "worst"][3] <= 1.0, by[cls, "worst"]
    assert mr["dropped tile 5"] > 1.0 and mr["dropped tile 11 (33 keys)"] > 1.0 and mr["stale tile 4"] > 1.0, mr


@pytest.mark.parametrize("cls", ["random", "flat"])
@pytest.mark.parametrize("t", [0, 5, 11])
def test_dropped_tile_is_rejected(cls, t):
    q, k, v, ref = case(cls)
    rejected(ref, emulate(q, k, v, drop=t))


@pytest.mark.parametrize("cls,t", [("random", 4), ("random", 11), ("peaked", 10)])
def test_stale_ring_buffer_is_rejected(cls, t):
    q, k, v, ref = case(cls)          # peaked: tile 10 is the last full tile and holds a third of the rows' dominant key
    rejected(ref, emulate(q, k, v, stale=t))


@pytest.mark.parametrize("cls", ["phantom", "flat"])
def test_phantom_key_is_rejected(cls):
    q, k, v, ref = case(cls)
    rejected(ref, emulate(q, k, v, phantom=True))


@pytest.mark.parametrize("block", [0, 2])
def test_missing_rescale_is_rejected(block):
    q, k, v, ref = case("peaked")
    O, m, l = emulate(q, k, v, skip_rescale=block)
    with pytest.raises(AssertionError):
        ref.check_o(normalise(O, l), "O")
    O2, m2, l2 = emulate(q, k, v)
    assert not torch.equal(m2, emulate(q, k[:64], v[:64])[1]), "no rescale fired: the class does not exercise the branch"


def test_merge_with_base_e_is_rejected():
    q, k, v, ref = case("random")
    cut = 6 * KVT
    parts = [emulate(q, k[:cut], v[:cut]), emulate(q, k[cut:], v[cut:])]
    assert ref.check_o(merge(parts), "2^") <= 1.0
    with pytest.raises(AssertionError):
        ref.check_o(merge(parts, base_e=True), "e^")
    # and against the fp64 merge of the same partials (the check of the merge kernel alone)
    po, pml = torch.stack([p[0] for p in parts])[:, :, None], torch.stack([torch.stack([p[1], p[2]], -1) for p in parts])[:, :, None]
    assert float(AB.merge_ratio(merge(parts), po, pml).max()) <= 1.0
    assert float(AB.merge_ratio(merge(parts, base_e=True), po, pml).max()) > 1.0


def test_unrounded_q_fails_the_contract_and_passes_its_own():
    """a test aid: the bound follows the operand values it is given - the kernel's q' is part of the contract"""
    q, k, v, ref = case("random")
    part = emulate(q, k, v, unrounded_q=True)
    rejected(ref, part)
    assert accepted(AB.AttnRef(q, k, v, H, rounded_q=False), part) <= 1.0


def test_data_classes_are_what_they_claim():
    for cls in AB.CLASSES:
        q, k, v, ref = case(cls)
        s = AB.q_prime(q).double() @ k.double().T
        if cls == "random":
            assert 1.6 < float(s.std()) < 2.4
        if cls == "flat":
            assert float(s.abs().max()) == 0.0
        if cls == "phantom":
            assert float(s.max()) < -30.0
        if cls == "peaked":
            top = s.argmax(dim=1)
            pos = AB.peak_positions(N_KV)
            assert pos == [5, 64 * 10 + 37, N_KV - 1]
            assert torch.equal(top, torch.tensor(pos)[torch.arange(N_Q) % 3])
            w = torch.softmax(s * math.log(2.0), dim=1).max(dim=1).values
            assert float(w.min()) > 0.99
