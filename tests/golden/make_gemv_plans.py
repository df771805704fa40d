"""Records what the quantized-GEMV dispatcher (exl3_gemv.hip) decides -- kernel generation and instantiation, split, waves, chunk, grid, LDS, workspace -- for the
requests the decode pipelines, the MoE path and LinearEXL3 really make, through the device-free query exl3_gemv_plan, into tests/golden/gemv_plans.json;
tests/test_gemv_plan.py replays it.

    python tests/golden/make_gemv_plans.py [--lib PATH/libexl3_hip.so]

The committed fixture is a recording of the dispatcher as it was BEFORE it was split into request / plan / launch (made from that commit's library with a
dry-run switch in its dispatcher, passed with --lib).  Regenerate it only with a change that means to alter dispatch and says so.

Layout: gemv_plans.json holds what a reader needs to name a request, gemv_plans.npz (int32 arrays) the bulk; load() joins them.
  rows     the row counts m a case is asked at: those up to its type's limit
  types    [name, [flags, operands, epi_mode, attm_hd, attm_nsplit, cpw, table slots or 0], most rows the validation admits]
  shapes   [k, [n, ...]]
  knobs    [variant, gemm3_min_rows, gemm3_cpw, gemv_gen4, max_waves, defer_wg_per_cu, tail_xcd_local] (index 0: the defaults)
  messages the dispatcher's refusals met in the cases
  invalid  requests the dispatcher refuses: [type entry, k, ns, m, K, cb, force_split, what, [rc, message]] (256 CUs, default knobs)
  npz: cases [type index, shape index, K, cb, num_cus, force_split, knobs index]; ids [case][row]: outcome index, -1 = not asked; outcomes
  [rc, first record in plans | message index, passes]; plans: one record of `fields` per pass
"""
import argparse
import ctypes
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "gemv_plans.json")
FIELDS = ["rows", "gen", "sel", "pre_xh", "S", "bps", "nwv", "chunk_blocks", "cpw", "grid_x", "grid_y", "grid_z", "lds", "ws_floats", "rows_per_pass",
          "xcd_local", "reduce"]
ROT, DEF, NORM, ATOMIC, FX, ACTFX = 1, 2, 4, 32, 64, 128                                     # exl3_gemv_args.h GEMV_*
XSUMS, TABLE, T_ACT_U, T_N_LIST, ACT, QKVM, RESID_IN, RESID_ALIAS, NO_SS_OUT = 1, 2, 4, 8, 16, 32, 64, 128, 256      # exl3_hip.h EXL3_PLAN_*
ROWS = [1, 2, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 144]      # edges of g4 / g2, g2 / g3 (rotated, raw), the 16- / 32- / 64-row passes, a multi-pass call

# name -> ([flags, operands, epi_mode, attm_hd, attm_nsplit, cpw, slots], most rows the validation admits, matrices it needs (0: any))
TYPES = {
    "plain": ([0, 0, 0, 0, 0, 0, 0], 144, 0),
    "raw_deferred": ([DEF, 0, 0, 0, 0, 0, 0], 16, 0),
    "rot_final": ([ROT, XSUMS, 0, 0, 0, 0, 0], 16, 0),
    "rot_deferred": ([ROT | DEF, 0, 0, 0, 0, 0, 0], 16, 0),
    "rot_deferred_xsums": ([ROT | DEF, XSUMS, 0, 0, 0, 0, 0], 16, 0),
    "norm_final": ([NORM, 0, 0, 0, 0, 0, 0], 16, 0),
    "norm_deferred": ([NORM | DEF, 0, 0, 0, 0, 0, 0], 16, 0),
    "fx": ([NORM | DEF | FX, 0, 0, 0, 0, 0, 0], 4, 0),
    "fx_atomic": ([NORM | ATOMIC | FX, 0, 0, 0, 0, 0, 0], 4, 0),
    "atomic_out": ([ATOMIC, 0, 0, 0, 0, 0, 0], 4, 0),
    "act_final": ([0, ACT, 0, 0, 0, 0, 0], 4, 1),
    "act_deferred": ([DEF, ACT, 0, 0, 0, 0, 0], 4, 1),
    "act_atomic": ([ATOMIC, ACT, 0, 0, 0, 0, 0], 4, 1),
    "act_rs_cpw4": ([DEF, ACT, 0, 0, 0, 4, 0], 4, 1),
    "actfx_atomic": ([ACTFX | ATOMIC, ACT, 0, 0, 0, 0, 0], 4, 1),
    "actfx_deferred": ([ACTFX | DEF, ACT, 0, 0, 0, 0, 0], 4, 1),
    "attm128_atomic": ([ATOMIC, 0, 0, 128, 8, 0, 0], 4, 1),
    "attm64_final": ([0, 0, 0, 64, 4, 0, 0], 4, 1),
    "qkvm_atomic": ([ATOMIC, QKVM, 0, 0, 0, 0, 0], 4, 1),
    "qkvm_deferred": ([DEF, QKVM, 0, 0, 0, 0, 0], 4, 1),
    "tail_norm": ([0, 0, 1, 0, 0, 0, 0], 16, 1),
    "tail_norm_rot": ([ROT, XSUMS, 1, 0, 0, 0, 0], 16, 1),
    "tail_act": ([0, 0, 2, 0, 0, 0, 0], 16, 2),
    "tail_act_rot": ([ROT, XSUMS, 2, 0, 0, 0, 0], 16, 2),
    "tail_qkv": ([0, 0, 3, 0, 0, 0, 0], 16, 3),
    "tail_qkv_rot": ([ROT, 0, 3, 0, 0, 0, 0], 16, 3),
    "tail_resid": ([0, 0, 4, 0, 0, 0, 0], 16, 1),
    "tail_resid_rot": ([ROT, XSUMS, 4, 0, 0, 0, 0], 16, 1),
    "resid_in_cpw4": ([NORM | DEF, RESID_IN, 0, 0, 0, 4, 0], 4, 0),
    "resid_in_cpw14": ([NORM | DEF, RESID_IN, 0, 0, 0, 14, 0], 4, 0),
    "wpc4": ([DEF, 0, 0, 0, 0, 4, 0], 4, 0),
    "wpc8": ([DEF, 0, 0, 0, 0, 8, 0], 4, 0),
}
for slots in (2, 4):                                                                          # Mixtral: 2 routed experts of a token, gate + up slots
    TYPES.update({
        f"table{slots}": ([0, TABLE, 0, 0, 0, 0, slots], 16, -1),
        f"table{slots}_act_u": ([0, TABLE | T_ACT_U, 0, 0, 0, 0, slots], 16, -1),
        f"table{slots}_n_list": ([0, TABLE | T_N_LIST, 0, 0, 0, 0, slots], 16, -1),
        f"table{slots}_deferred": ([DEF, TABLE, 0, 0, 0, 0, slots], 4, -1),
        f"table{slots}_act_deferred": ([DEF, TABLE | T_ACT_U, 0, 0, 0, 0, slots], 4, -1),
        f"table{slots}_act_fx": ([ATOMIC, TABLE | ACT, 0, 0, 0, 0, slots], 4, -1),
    })


def model_shapes(hidden, inter, q, kv, vocab):
    return [(hidden, [q, kv, kv]), (q, [hidden]), (hidden, [inter, inter]), (inter, [hidden]), (hidden, [vocab])]


LLAMA_8B = model_shapes(4096, 14336, 4096, 1024, 128256)
TINY_A, TINY_B = model_shapes(256, 512, 256, 128, 384), model_shapes(512, 1024, 512, 256, 384)
OTHERS = model_shapes(2048, 8192, 2048, 512, 128256) + [(8192, [1024, 128, 128]), (1024, [8192]), (8192, [3584, 3584]), (3584, [8192])]      # Llama-3.2-1B, a 70B TP = 8 shard
MIXTRAL = [(4096, [14336]), (14336, [4096])]
DEFAULT_KNOBS = [1, 5, 0, 1, 0, 0, 0]
KNOBS = [DEFAULT_KNOBS]
for pos, values in ((1, [0]), (2, [1, 2, 4]), (3, [0]), (4, [4, -8]), (5, [2]), (6, [1])):    # one knob at a time
    for v in values:
        KNOBS.append(DEFAULT_KNOBS[:pos] + [v] + DEFAULT_KNOBS[pos + 1:])
VARIANT0 = len(KNOBS)
KNOBS.append([0] + DEFAULT_KNOBS[1:])

# the dispatcher refuses these: (type entry, k, ns, m, K, cb, force_split, what)
INVALID = [
    ([ROT | DEF, 0, 0, 0, 0, 0, 0], 4096, [4096], 17, 4, 2, 0, "17 deferred rows"),
    ([0, 0, 0, 0, 0, 0, 0], 192, [256], 1, 4, 2, 0, "k = 192"),
    ([0, 0, 0, 0, 0, 0, 0], 256, [100], 1, 4, 2, 0, "n = 100"),
    ([DEF, 0, 0, 0, 0, 17, 0], 4096, [4096], 1, 4, 2, 0, "cpw 17"),
    ([ROT | DEF, 0, 0, 0, 0, 4, 0], 4096, [4096], 1, 4, 2, 0, "cpw with rotated input"),
    ([0, 0, 0, 0, 0, 0, 0], 4096, [4096], 1, 9, 2, 0, "K = 9"),
    ([ATOMIC, 0, 0, 0, 0, 0, 0], 4096, [4096], 5, 4, 2, 0, "atomic out with 5 rows"),
    ([ATOMIC, 0, 0, 128, 8, 0, 0], 4096, [4096, 4096], 1, 4, 2, 0, "ATTM with two matrices"),
    ([NORM | DEF | FX, NO_SS_OUT, 0, 0, 0, 0, 0], 4096, [4096], 1, 4, 2, 0, "fixed-point input without ss_out"),
    ([NORM | DEF, RESID_IN | RESID_ALIAS, 0, 0, 0, 4, 0], 4096, [4096], 1, 4, 2, 0, "RESID input with resid_out == resid_in"),
    ([0, 0, 4, 0, 0, 0, 0], 256, [128 * 65536], 1, 4, 2, 0, "a tail with more column blocks than tickets"),
    ([0, 0, 4, 0, 0, 0, 0], 128 * 256, [128], 1, 4, 2, 256, "a tail split deeper than 128"),
    ([DEF, 0, 0, 0, 0, 4, 0], 14336, [4096], 4, 4, 0, 1, "a wave-per-column-block slice beyond one LDS chunk"),
    ([NORM | DEF | FX, 0, 0, 0, 0, 0, 0], 14336, [4096], 1, 4, 2, 2, "a fixed-point launch generation 4 cannot take (56-block slices)"),
]


def case_list():
    """(shapes, [type index, shape index, K, cb, num_cus, force_split, knobs index]): the shapes the pipelines launch x the call types they admit."""
    shapes, cases = [], []

    def shape_id(sh):
        sh = [sh[0], list(sh[1])]
        if sh not in shapes: shapes.append(sh)
        return shapes.index(sh)

    def add(group, K, cb, cus, fs=0, knobs=0, types=None):
        for sh in group:
            for name, (entry, max_m, mats) in TYPES.items():
                if types is not None and name not in types: continue
                if (mats == -1) != (group is MIXTRAL) or (mats > 0 and mats != len(sh[1])): continue
                cases.append([list(TYPES).index(name), shape_id(sh), K, cb, cus, fs, knobs])

    kcv = [(K, cb, v) for K in (1, 3, 4, 5, 8) for cb in (0, 2) for v in (1, 0)]
    some = [(4, 2, 1), (5, 0, 1), (1, 2, 0), (8, 0, 0), (3, 2, 1)]                           # every K, both codebooks, both variants
    # (the full product of every axis would be half a million requests: K x codebook x variant is full on the 8B shapes at
    # 256 CUs, and thinned elsewhere -- every value of every axis still meets every call type, shape and row count)
    for cus, full, thin in ((256, kcv, some), (304, some[:3], some[:1]), (64, some[:3], some[:1])):
        for K, cb, v in full:
            add(LLAMA_8B, K, cb, cus, knobs=VARIANT0 if v == 0 else 0)
        for K, cb, v in thin:
            add(OTHERS + TINY_A + TINY_B, K, cb, cus, knobs=VARIANT0 if v == 0 else 0)
            add(MIXTRAL, K, cb, cus, knobs=VARIANT0 if v == 0 else 0)
    for fs in (3, 8, 100):
        add(LLAMA_8B, 4, 2, 256, fs=fs)
    for kn in range(1, VARIANT0):
        add(LLAMA_8B, 4, 2, 256, knobs=kn)
        add(LLAMA_8B, 5, 0, 256, knobs=kn, types=("plain", "rot_deferred", "norm_final", "act_final", "tail_resid", "tail_norm"))
    return shapes, cases


SETTERS = ("exl3_set_gemv_variant", "exl3_set_gemm3_min_rows", "exl3_set_gemm3_cpw", "exl3_set_gemv_gen4", "exl3_set_gemv_max_waves",
           "exl3_set_gemv_defer_wg_per_cu")


class Planner:
    """exl3_gemv_plan of a library, with the tuning hooks of a knobs entry applied (tail_xcd_local goes in through the query: its setter probes a device)."""

    def __init__(self, lib):
        self.lib, self.knobs = lib, None
        lib.exl3_last_error.restype = ctypes.c_char_p
        self.out = (ctypes.c_int32 * (len(FIELDS) * 16))()
        self.passes = ctypes.c_int(0)

    def set_knobs(self, knobs):
        if knobs != self.knobs:
            for name, v in zip(SETTERS, knobs): getattr(self.lib, name)(ctypes.c_int(v))
            self.knobs = list(knobs)

    def outcome(self, entry, k, ns, m, K, cb, cus, fs):
        flags, operands, epi, hd, nsplit, cpw, slots = entry
        rc = self.lib.exl3_gemv_plan(flags, (ctypes.c_int * len(ns))(*ns), slots or len(ns), m, k, K, cb, fs, cpw, operands, epi, hd, nsplit, cus,
                                     self.knobs[6], self.out, 16, ctypes.byref(self.passes))
        if rc != 0:
            return [rc, self.lib.exl3_last_error().decode()]
        w = len(FIELDS)
        return [0, [list(self.out[i * w:(i + 1) * w]) for i in range(self.passes.value)]]


def record(planner):
    """(the JSON part, the arrays of the npz part)"""
    import numpy as np
    shapes, cases = case_list()
    types = [[n, t[0], t[1]] for n, t in TYPES.items()]
    plans, messages, outcomes, index = [], [], [], {}

    def oid(o):
        key = json.dumps(o)
        if key not in index:
            index[key] = len(outcomes)
            if o[0] != 0:
                if o[1] not in messages: messages.append(o[1])
                outcomes.append([o[0], messages.index(o[1]), 0])
            else:
                outcomes.append([0, len(plans), len(o[1])]); plans.extend(o[1])
        return index[key]

    ids = np.full((len(cases), len(ROWS)), -1, dtype=np.int32)
    try:
        for i, (ti, sh, K, cb, cus, fs, kn) in enumerate(cases):
            entry, max_m = types[ti][1:]
            planner.set_knobs(KNOBS[kn])
            for j, m in enumerate(ROWS):
                if m <= max_m: ids[i, j] = oid(planner.outcome(entry, shapes[sh][0], shapes[sh][1], m, K, cb, cus, fs))
        planner.set_knobs(DEFAULT_KNOBS)
        invalid = [[entry, k, ns, m, K, cb, fs, what, planner.outcome(entry, k, ns, m, K, cb, 256, fs)] for entry, k, ns, m, K, cb, fs, what in INVALID]
    finally:
        planner.set_knobs(DEFAULT_KNOBS)
    head = {"fields": FIELDS, "rows": ROWS, "types": types, "shapes": shapes, "knobs": KNOBS, "messages": messages, "invalid": invalid}
    arrays = {"cases": np.array(cases, dtype=np.int32), "ids": ids, "outcomes": np.array(outcomes, dtype=np.int32), "plans": np.array(plans, dtype=np.int32)}
    return head, arrays


def load(golden_dir):
    """The recording as record() made it, outcomes back in the form Planner.outcome returns: (head, cases, ids, outcomes)."""
    import numpy as np
    with open(os.path.join(golden_dir, "gemv_plans.json")) as f:
        head = json.load(f)
    a = np.load(os.path.join(golden_dir, "gemv_plans.npz"))
    plans = a["plans"].tolist()
    outcomes = [[rc, head["messages"][first]] if rc != 0 else [0, plans[first:first + n]] for rc, first, n in a["outcomes"].tolist()]
    return head, a["cases"].tolist(), a["ids"].tolist(), outcomes


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="libexl3_hip.so to record from (default: this tree's)")
    a = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401  (before the library: exllamav3_amd/_lib.py explains)
    if a.lib:
        lib = ctypes.CDLL(a.lib, mode=ctypes.RTLD_GLOBAL)
    else:
        import sys
        sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
        from exllamav3_amd import _lib
        lib = _lib.lib()
    head, arrays = record(Planner(lib))
    with open(OUT, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" if not isinstance(v, list) or k in ("fields", "rows") else
                                  json.dumps(k) + ": [\n  " + ",\n  ".join(json.dumps(x) for x in v) + "\n]" for k, v in head.items()) + "\n}\n")
    np.savez_compressed(OUT[:-5] + ".npz", **arrays)
    print(f"{len(arrays['cases'])} case rows, {int((arrays['ids'] >= 0).sum())} requests, {len(arrays['outcomes'])} distinct outcomes, {len(head['invalid'])} refused -> "
          f"{OUT} ({os.path.getsize(OUT)} bytes) + .npz ({os.path.getsize(OUT[:-5] + '.npz')} bytes)")
