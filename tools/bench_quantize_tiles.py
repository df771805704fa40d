"""Throughput of the trellis encoder (exl3_quantize_tiles.kspec.hip) on one GPU.

For each K x codebook: >= 4096 seeded randn x codebook-RMS tiles, one warm-up launch sequence, then device-event timing of
exllamav3_amd.quantize.quantize_tiles.  Reports tiles/s, candidate evaluations/s (tiles x 2 passes x 256 positions x 65536 candidates / time)
against the VALU bound, the VALU instructions per evaluation counted in the inner loop's ISA (build/obj, CPU side), and the time of
encode_linear on 4096 x 4096 and 4096 x 14336 at K = 4.

    python tools/bench_quantize_tiles.py [--tiles 4096] [--out profiles/quantize_tiles_bench.json] [--ks 1,2,...] [--isa-only]
"""
from __future__ import annotations
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LLVM = "/opt/rocm/lib/llvm/bin"
CB_NAMES = {0: "3inst", 1: "mcg", 2: "mul1"}
VALU_LANE_OPS_PER_S = 256 * 4 * 16 * 2.4e9        # 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz


def _disassemble(obj: str) -> str:
    with tempfile.TemporaryDirectory() as td:
        fat, co = os.path.join(td, "fat.bin"), os.path.join(td, "dev.co")
        subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True, capture_output=True)
        return subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout


def ins_raw(body: str):
    for l in body.splitlines():
        a_ = re.search(r"//\s*([0-9A-Fa-f]+):", l)
        if a_:
            yield int(a_.group(1), 16), l


def inner_loop_valu_per_eval(K: int) -> dict:
    """VALU instructions per candidate evaluation in the steady-state step body: the loop with LDS cost reads whose body holds the most
    v_pk_fma_f16 in each codebook's kernel; candidate pairs counted by their v_pk_add_f16; per evaluation = VALU per candidate pair / 2."""
    obj = os.path.join(ROOT, "build", "obj", f"exl3_quantize_tiles_k{K}.o")
    if not os.path.exists(obj):
        return {}
    text = _disassemble(obj)
    out = {}
    for base, name, body in re.findall(r"^([0-9a-f]+) <(\S+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", text, flags=re.S | re.M):
        m = re.search(r"exl3_quantize_tiles_kernelILi\d+ELi(\d)E", name)
        if not m:
            continue
        cb, base = int(m.group(1)), int(base, 16)
        ins = []                                                           # (address, text)
        for l in body.splitlines():
            a_ = re.search(r"//\s*([0-9A-Fa-f]+):", l)
            if a_:
                ins.append((int(a_.group(1), 16), l.split("//")[0].strip()))
        # loops = backward branches; the step loop is the one with the most v_pk_fma_f16 (one per candidate pair; mul1: two)
        best = None
        for addr, l in ins:
            b = re.search(r"^s_(?:cbranch_\w+|branch)\b", l)
            t_ = re.search(r"<\S+\+0x([0-9a-f]+)>", dict(ins_raw(body)).get(addr, "")) if b else None
            if not t_:
                continue
            tgt = base + int(t_.group(1), 16)
            if tgt > addr:
                continue
            seg = [x for a2, x in ins if tgt <= a2 <= addr]
            fma = sum(1 for x in seg if x.startswith("v_pk_fma_f16"))
            if fma and any(x.startswith("ds_read") for x in seg) and (best is None or fma > best[0]):
                valu = sum(1 for x in seg if x.startswith("v_"))
                adds = sum(1 for x in seg if x.startswith("v_pk_add_f16"))
                best = (fma, valu, len(seg), adds)
        if best:
            fma, valu, n, adds = best
            pairs = adds // 2 if cb != 2 else adds              # per candidate pair: decode add + delta (3INST / mcg), delta (mul1)
            out[CB_NAMES[cb]] = {"valu_per_eval": round(valu / pairs / 2, 2), "loop_valu": valu, "loop_instructions": n, "candidate_pairs": pairs}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=4096)
    ap.add_argument("--ks", default="1,2,3,4,5,6,7,8")
    ap.add_argument("--out", default=None)
    ap.add_argument("--isa-only", action="store_true")
    ap.add_argument("--skip-linear", action="store_true")
    a = ap.parse_args()
    ks = [int(k) for k in a.ks.split(",")]
    res = {"isa": {k: inner_loop_valu_per_eval(k) for k in ks}}
    if a.isa_only:
        print(json.dumps(res, indent=1))
        return
    import torch
    from exllamav3_amd import ext, quantize
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res["device"] = torch.cuda.get_device_name(dev)
    res["num_cus"] = ext.g_get_num_sms(0)
    g = torch.Generator(device=dev).manual_seed(0)
    rates = []
    for K in ks:
        for cb, (mcg, mul1) in enumerate([(False, False), (True, False), (False, True)]):
            scale = 1.0 if cb == 2 else quantize.CODEBOOK_SCALE
            x = torch.randn((a.tiles, 256), generator=g, device=dev) * scale
            quantize.quantize_tiles(x[:quantize.batch_tiles(K, dev)], K, mcg, mul1)         # warm-up: one full batch
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out, idx = quantize.quantize_tiles(x, K, mcg, mul1)
            e1.record()
            torch.cuda.synchronize()
            s = e0.elapsed_time(e1) / 1e3
            evals = a.tiles * 2 * 256 * 65536 / s
            mse = ((out - x) / scale).pow(2).mean().item()
            isa = res["isa"].get(K, {}).get(CB_NAMES[cb], {})
            row = {"K": K, "cb": CB_NAMES[cb], "tiles": a.tiles, "seconds": round(s, 5), "tiles_per_s": round(a.tiles / s, 1),
                   "evals_per_s": float(f"{evals:.4g}"), "nmse": round(mse, 5)}
            if isa:
                bound = VALU_LANE_OPS_PER_S / isa["valu_per_eval"]
                row["valu_per_eval"] = isa["valu_per_eval"]
                row["valu_bound_evals_per_s"] = float(f"{bound:.4g}")
                row["share_of_valu_bound"] = round(evals / bound, 3)
            print(json.dumps(row), flush=True)
            rates.append(row)
    res["rates"] = rates
    if not a.skip_linear:
        lin = []
        for (k, n) in [(4096, 4096), (4096, 14336)]:
            w = torch.randn((k, n), generator=g, device=dev) * 0.02
            quantize.encode_linear(w[:, :1024].contiguous(), 4)                # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            quantize.encode_linear(w, 4)
            torch.cuda.synchronize()
            row = {"k": k, "n": n, "K": 4, "cb": "3inst", "seconds": round(time.perf_counter() - t0, 3), "tiles": k * n // 256}
            print(json.dumps(row), flush=True)
            lin.append(row)
        res["encode_linear"] = lin
    if a.out:
        os.makedirs(os.path.dirname(os.path.join(ROOT, a.out)), exist_ok=True)
        json.dump(res, open(os.path.join(ROOT, a.out), "w"), indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
