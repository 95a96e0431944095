#!/usr/bin/env python3
"""Write the candidate temporal-op configurations of the VAE study, one exp_<n>.json per candidate (numbered from 1), from a base
t_ops_config.json.  One tool for the fork's three enumeration scripts:

  --mode pool     all switches off, then exactly one encoder pooling slot x one decoder interpolation slot on.  Slots are ordered
                  (block, resnet index, before/after) over encoder.down_blocks and decoder.up_blocks (the mid block is not
                  enumerated); at most 384 files.
  --mode stride   the temporal stride of one encoder downsampler doubled (block 0: [1,2,2] -> [2,2,2]; blocks 1, 2: first entry
                  doubled) x one decoder slot.
  --mode stride2  two of those three downsamplers x two decoder slots.

Usage: python dynamic_enumeration.py <config.json> [output_dir] [--mode pool|stride|stride2]"""
import argparse
import copy
import json
import os
from itertools import combinations

MAX_COMBOS = 384
STRIDE_BLOCKS = (0, 1, 2)


def _slots(blocks, before_key, after_key):
    out = []
    for i, block in enumerate(blocks):
        for j in range(min(len(block.get(before_key, [])), len(block.get(after_key, [])))):
            out.append((i, j, "before"))
            out.append((i, j, "after"))
    return out


def encoder_slots(config):
    return _slots(config.get("encoder", {}).get("down_blocks", []), "enable_t_pool_before_block", "enable_t_pool_after_block")


def decoder_slots(config):
    return _slots(config.get("decoder", {}).get("up_blocks", []), "enable_t_interp_before_block", "enable_t_interp_after_block")


def _clear(blocks, keys):
    for block in blocks:
        for k in keys:
            if k in block:
                block[k] = [False] * len(block[k])


def clear_encoder(config):
    _clear(config.get("encoder", {}).get("down_blocks", []), ("enable_t_pool_before_block", "enable_t_pool_after_block"))


def clear_decoder(config):
    _clear(config.get("decoder", {}).get("up_blocks", []), ("enable_t_interp_before_block", "enable_t_interp_after_block"))


def _switch_on(block, prefix, slot):
    _, j, pos = slot
    block[f"{prefix}_{pos}_block"][j] = True


def double_temporal_stride(config, block_idx):
    block = config["encoder"]["down_blocks"][block_idx]
    s = block["downsample_stride"]
    block["downsample_stride"] = [2 if block_idx == 0 else s[0] * 2, s[1], s[2]]


def enumerate_configs(base, mode="pool"):
    """yields (config, description) in file order"""
    dec = decoder_slots(base)
    if mode == "pool":
        n = 0
        for e in encoder_slots(base):
            for d in dec:
                n += 1
                if n > MAX_COMBOS:
                    return
                cfg = copy.deepcopy(base)
                clear_encoder(cfg), clear_decoder(cfg)
                _switch_on(cfg["encoder"]["down_blocks"][e[0]], "enable_t_pool", e)
                _switch_on(cfg["decoder"]["up_blocks"][d[0]], "enable_t_interp", d)
                yield cfg, f"enc={e}, dec={d}"
    elif mode in ("stride", "stride2"):
        k = 1 if mode == "stride" else 2
        for blocks in combinations(STRIDE_BLOCKS, k):
            for ds in combinations(dec, k):
                cfg = copy.deepcopy(base)
                for b in blocks:
                    double_temporal_stride(cfg, b)
                clear_encoder(cfg), clear_decoder(cfg)
                for d in ds:
                    _switch_on(cfg["decoder"]["up_blocks"][d[0]], "enable_t_interp", d)
                yield cfg, f"encoder_blocks={blocks}, dec={ds}"
    else:
        raise ValueError(f"unknown mode {mode!r}: pool, stride or stride2")


def write_configs(config_path, output_dir, mode="pool", limit=None):
    with open(config_path, "r") as f:
        base = json.load(f)
    os.makedirs(output_dir, exist_ok=True)
    paths = []
    for n, (cfg, what) in enumerate(enumerate_configs(base, mode), start=1):
        if limit is not None and n > limit:
            break
        path = os.path.join(output_dir, f"exp_{n}.json")
        with open(path, "w") as f:
            json.dump(cfg, f, indent=2)
        paths.append(path)
        print(f"[INFO] Wrote {path}, ({what})")
    return paths


def main(argv=None):
    p = argparse.ArgumentParser(description="Enumerate temporal-op configurations of the VAE study.")
    p.add_argument("config", help="base t_ops_config.json")
    p.add_argument("output_dir", nargs="?", default=None, help="default: config_<mode>_json next to the base config")
    p.add_argument("--mode", choices=("pool", "stride", "stride2"), default="pool")
    a = p.parse_args(argv)
    out = a.output_dir or os.path.join(os.path.dirname(os.path.abspath(a.config)), f"config_{a.mode}_json")
    paths = write_configs(a.config, out, a.mode)
    print(f"[INFO] Done: {len(paths)} configurations in {out}")
    return paths


if __name__ == "__main__":
    main()
