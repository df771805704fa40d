#!/usr/bin/env python3
"""Records the outputs of the reference libraries in oracle/_ref (built by oracle/build_ref.sh where the reference sources lie) for every case of the
tests in tests/test_oracle_pins.py that call them, as tests/golden/ref_kernels_part*.npz: the record those tests read where oracle/_ref is absent.

Every test is run here with the live libraries (so the oracle is checked against them on the way); each case's outputs go into the record, arrays
above 64 KiB as SHA-256 digests of their bytes, dtype and shape.  Where the libraries exist the tests also check them against this record.

Run from the repository root after build():  python tests/golden/make_ref_kernels.py        (no GPU)
"""
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]

import test_oracle_pins as T  # noqa: E402
from npz_parts import save_parts  # noqa: E402

TESTS = ["test_format_against_reference_cpu_impl", "test_codebooks_all_states_against_reference_device_code",
         "test_window_readers_against_reference_device_code", "test_kv_quant_against_reference_device_code",
         "test_kv_paged_addressing_against_reference_kernels", "test_kv_compander_against_reference_device_code",
         "test_kv_paged_sliding_window_and_window_scratch_against_reference_kernels", "test_act_mul_against_reference_kernels",
         "test_attention_gates_against_reference_kernels"]


def cases(fn):
    """Every argument combination of the function's parametrize marks."""
    axes = []
    for m in getattr(fn, "pytestmark", []):
        if m.name != "parametrize":
            continue
        names = [a.strip() for a in m.args[0].split(",")]
        axes.append([dict(zip(names, v if len(names) > 1 else (v,))) for v in m.args[1]])
    for combo in itertools.product(*axes):
        kw = {}
        for d in combo:
            kw.update(d)
        yield kw


def main():
    missing = [f for f in T._REF_LIBS.values() if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", f))]
    if missing:
        sys.exit(f"oracle/_ref lacks {missing}: run build() where the reference sources are present")
    T._RECORDING = {}
    for name in TESTS:
        for kw in cases(getattr(T, name)):
            getattr(T, name)(**kw)
    arrays, digests = {}, {}
    for case, outs in T._RECORDING.items():
        for k, a in outs.items():
            if a.nbytes > T._DIGEST_ABOVE:
                digests[f"{case}/{k}"] = T._digest(a)
            else:
                arrays[f"{case}/{k}"] = a
    arrays["digests"] = np.frombuffer(json.dumps(digests, sort_keys=True).encode(), dtype=np.uint8)
    paths = save_parts(os.path.join(HERE, "ref_kernels"), arrays)
    print(f"wrote {paths}: {len(T._RECORDING)} cases, {len(arrays) - 1} arrays, {len(digests)} digests")


if __name__ == "__main__":
    main()
