#!/usr/bin/env python3
"""Phase stamps of the persistent decode step, the streaming waves grouped BY SIMD (waves w, w + 4, w + 8 share SIMD w % 4): for gate|up, down and the lm_head, the
median over layers and workgroups of when each streaming wave was done (slot 16 + w) after the LAST service wave published the input quads (slots 28..31), and per
SIMD the time its last wave was done -- the streaming phase ends with the fullest SIMD (exl3_pstep.hip: wave_partition).  Stamps file: tools/experiments/pstep_harness.hip
(argument 5), [op][cu][32] x u64 at 100 MHz; tools/pstep_stamps.py reads the same file by phase.
usage: tools/pstep_simd_stamps.py <stamps.bin> <layers> [json out]"""
import json
import sys
import numpy as np


def by_simd(a, ops):
    qp, fin = a[ops][:, :, 28:32], a[ops][:, :, 16:28]
    have = (fin > 0).all(axis=2) & (qp > 0).all(axis=2)
    if not have.any():
        return None
    rel = ((fin - qp.max(axis=2, keepdims=True))[have]) / 100.0               # [samples][wave], microseconds
    waves = [round(float(np.median(rel[:, w])), 2) for w in range(12)]
    last = [round(float(np.median(rel[:, s::4].max(axis=1))), 2) for s in range(4)]
    return {"samples": int(have.sum()), "simd_waves_done_after_quads_us": {"simd%d" % s: waves[s::4] for s in range(4)},
            "simd_last_wave_done_after_quads_us": last, "all_waves_done_after_quads_us": round(float(np.median(rel.max(axis=1))), 2),
            "slowest_simd_share": [round(float(np.mean(rel[:, s::4].max(axis=1) >= rel.max(axis=1))), 3) for s in range(4)]}


def main():
    path, nl = sys.argv[1], int(sys.argv[2])
    a = np.fromfile(path, dtype=np.uint64)
    nops = 4 * nl + 1
    ncu = a.size // (nops * 32)
    a = a[:nops * ncu * 32].reshape(nops, ncu, 32).astype(np.int64)
    out = {"workgroups": int(ncu), "layers": nl, "ops": {}}
    kinds = {"gate_up": [4 * l + 2 for l in range(1, nl)], "down": [4 * l + 3 for l in range(1, nl)], "head": [nops - 1]}
    for name, ops in kinds.items():
        if not ops: continue
        rec = by_simd(a, ops)
        out["ops"][name] = rec
        if rec is None:
            print(f"{name}: no stamps"); continue
        print(f"{name}: all waves done {rec['all_waves_done_after_quads_us']} us after the quads; last wave per SIMD {rec['simd_last_wave_done_after_quads_us']}; "
              f"share of rectangles a SIMD ends last {rec['slowest_simd_share']}")
        for s in range(4): print(f"    SIMD {s} (waves {s}, {s + 4}, {s + 8}): {rec['simd_waves_done_after_quads_us']['simd%d' % s]}")
    if len(sys.argv) > 3:
        json.dump(out, open(sys.argv[3], "w"), indent=1)


if __name__ == "__main__":
    main()
