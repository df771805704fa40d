"""What the quantized-GEMV dispatcher decides (exl3_gemv.hip: gemv_validate / gemv_plan_pass through the device-free query exl3_gemv_plan, no GPU): kernel
generation and instantiation, pre-rotation, split, waves per workgroup, chunk, column blocks per workgroup, grid, LDS bytes, workspace floats, the tail
epilogue's rows per pass and hand-off, the reduce launch -- field for field what the fixture (tests/golden/gemv_plans.json + gemv_plans.npz, joined by
make_gemv_plans.load) holds for every request in it, and for the requests the dispatcher refuses the same return code and message.

The fixture is a RECORDING OF THE PRE-REFACTOR DISPATCHER (the monolithic run_mgemm, run with a dry-run switch on the shapes the decode pipelines, the MoE
path and LinearEXL3 launch: tests/golden/make_gemv_plans.py), not an output of the code under test.  The GPU parity tests compare against the oracle at a
tolerance, so a drifted split passes them and shows only as a slower benchmark line; this test is what pins the tuned choices.  Regenerate the fixture
only with a change that means to alter dispatch and says so."""
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def mk():
    sys.path.insert(0, GOLDEN)
    try:
        import make_gemv_plans
    finally:
        sys.path.remove(GOLDEN)
    return make_gemv_plans


@pytest.fixture(scope="module")
def recording(mk):
    head, cases, ids, outcomes = mk.load(GOLDEN)
    return dict(head, cases=[c + [[i for i in row if i >= 0]] for c, row in zip(cases, ids)], outcomes=outcomes)


@pytest.fixture(scope="module")
def planner(mk):
    from exllamav3_amd import _lib
    p = mk.Planner(_lib.lib())
    yield p
    p.set_knobs(mk.DEFAULT_KNOBS)


def test_every_recorded_request_plans_as_recorded(recording, planner):
    r = recording
    fields, rows, outcomes = r["fields"], r["rows"], r["outcomes"]
    bad = []
    try:
        for ti, sh, K, cb, cus, fs, kn, ids in r["cases"]:
            name, entry, max_m = r["types"][ti]
            k, ns = r["shapes"][sh]
            planner.set_knobs(r["knobs"][kn])
            ms = [m for m in rows if m <= max_m]
            assert len(ms) == len(ids)
            for m, oi in zip(ms, ids):
                got, want = planner.outcome(entry, k, ns, m, K, cb, cus, fs), outcomes[oi]
                if got != want and len(bad) < 20:
                    bad.append((name, k, ns, m, K, cb, cus, fs, r["knobs"][kn], _diff(fields, got, want)))
    finally:
        planner.set_knobs(r["knobs"][0])
    assert not bad, "\n".join(map(str, bad))


def _diff(fields, got, want):
    if got[0] != 0 or want[0] != 0 or len(got[1]) != len(want[1]):
        return ("got", got, "recorded", want)
    return [(i, f, g, w) for i, (pg, pw) in enumerate(zip(got[1], want[1])) for f, g, w in zip(fields, pg, pw) if g != w]


def test_refused_requests_keep_their_code_and_message(recording, planner):
    planner.set_knobs(recording["knobs"][0])
    assert len(recording["invalid"]) >= 12
    for entry, k, ns, m, K, cb, fs, what, want in recording["invalid"]:
        assert want[0] < 0 and isinstance(want[1], str) and want[1], what
        assert planner.outcome(entry, k, ns, m, K, cb, 256, fs) == want, what


def test_the_recording_reaches_every_kernel_family(recording):
    """(generation, instantiation) pairs the fixture must contain: generation 4 modes 0..9; generation 2 at ng 1 / 2 / 4, with each tail epilogue, in the
    wave-per-column-block layout and as a table launch; generation 3 at mt 1 / 2 / 4, each with and without the pre-rotation."""
    r = recording
    f = {n: i for i, n in enumerate(r["fields"])}
    seen = set()
    for ti, sh, K, cb, cus, fs, kn, ids in r["cases"]:
        name, (flags, operands, epi, hd, nsplit, cpw, slots), max_m = r["types"][ti]
        for oi in ids:
            rc, plans = r["outcomes"][oi]
            if rc != 0: continue
            for p in plans:
                gen, sel = p[f["gen"]], p[f["sel"]]
                seen.add((gen, sel))
                if gen == 3: seen.add((3, sel, "pre_xh" if p[f["pre_xh"]] else "in place"))
                if gen == 2 and epi: seen.add((2, "epi", epi))
                if gen == 2 and p[f["cpw"]] > 0: seen.add((2, "wpc"))
                if gen == 2 and slots: seen.add((2, "table"))
    need = {(4, mode) for mode in range(10)} | {(2, ng) for ng in (1, 2, 4)} | {(2, "epi", e) for e in (1, 2, 3, 4)} | {(2, "wpc"), (2, "table")}
    need |= {(3, mt, how) for mt in (1, 2, 4) for how in ("pre_xh", "in place")}
    assert not need - seen, sorted(map(str, need - seen))


def test_ext_wrapper_names_the_fields(recording):
    from exllamav3_amd import ext
    assert list(ext.GEMV_PLAN_FIELDS) == recording["fields"]
    plans = ext.gemv_plan([4096, 1024, 1024], m=1, k=4096, K=4, cb=2, num_cus=256, flags=2)
    assert len(plans) == 1 and plans[0]["rows"] == 1 and plans[0]["gen"] == 4 and plans[0]["grid_x"] == plans[0]["S"] and plans[0]["grid_y"] == 48
    with pytest.raises(RuntimeError, match="k must be divisible by 128"):
        ext.gemv_plan([256], m=1, k=192, K=4, cb=2, num_cus=256)
