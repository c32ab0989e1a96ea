"""Which kernel a layout gets, checked without a GPU (tools/dispatch_record.py): cz_kernels.hip compiled
host-only under a shim that prints every launch instead of making it, driven over base and stride
phases, stride and length limits, counts and knob settings.  tests/golden/dispatch_parent.txt is the
record of the launchers as they were before they were rebuilt on the pure plan of cz_dispatch.h; the
working tree must record the same text -- the same instantiation, grid, LDS bytes, arguments and
zero-pad launch for every case.  CPU only (hipcc compiles the host side)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dispatch_record  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "dispatch_parent.txt")
needs_hipcc = pytest.mark.skipif(not os.path.exists(dispatch_record.HIPCC), reason="hipcc not installed")

ST = {"DIRECT": 0, "LINES": 1, "REGION": 2, "SHIFT": 3}
MODE_ZMQ, MODE_BOX = 0, 2


def _inst(name, sts, pair, *rest):
    return {f"{name}<{ST[s]},{'true' if pair else 'false'}{''.join(f',{r}' for r in rest)}>" for s in sts}


# every instantiation the launchers may launch, and no other
INSTANTIATIONS = (
    # uniform seal
    _inst("k_seal_uniform", ["LINES", "SHIFT", "DIRECT"], True, MODE_ZMQ)
    | _inst("k_seal_uniform", ["LINES", "REGION", "SHIFT", "DIRECT"], False, MODE_ZMQ)
    | _inst("k_seal_uniform_ina", ["LINES", "SHIFT"], True, 8) | _inst("k_seal_uniform_ina", ["LINES", "SHIFT"], True, 1)
    | _inst("k_seal_uniform_ina", ["REGION"], False, 8) | _inst("k_seal_uniform_ina", ["REGION"], False, 1)
    # box seal
    | _inst("k_seal_uniform", ["LINES", "DIRECT"], True, MODE_BOX)
    # fan-out, fan-out runs
    | {f"{k}<{ST[s]},{p}>" for k in ("k_seal_fanout", "k_seal_fanout_runs")
       for s, p in (("LINES", "true"), ("REGION", "false"), ("DIRECT", "true"))}
    # uniform open
    | _inst("k_open_uniform", ["LINES", "DIRECT"], True, 16)
    | _inst("k_open_uniform", ["LINES", "REGION", "DIRECT"], False, 16)
    | _inst("k_open_uniform", ["LINES"], True, 8) | _inst("k_open_uniform", ["LINES"], True, 1)
    | _inst("k_open_uniform", ["SHIFT"], True, 16) | _inst("k_open_uniform", ["SHIFT"], True, 8)
    | _inst("k_open_uniform", ["SHIFT"], True, 1)
    | _inst("k_open_uniform", ["REGION"], False, 8) | _inst("k_open_uniform", ["REGION"], False, 1)
    | {"k_open_uniform_carry<8>", "k_open_uniform_carry<1>"}
    # the rest of owned slots, the segment launchers
    | {"k_zero_pad", "k_seal_segments_lines", "k_seal_segments", "k_seal_combine", "k_open_segments", "k_open_combine"}
)


def test_normalise_two_spellings_of_one_instantiation():
    n = dispatch_record.normalise_kernel
    assert n("(k_seal_uniform<ST_LINES, true>)") == n("(k_seal_uniform<ST_LINES, true, MODE_ZMQ>)") == "k_seal_uniform<1,true,0>"
    assert n("(k_seal_uniform<ST_DIRECT, true, MODE_BOX>)") == "k_seal_uniform<0,true,2>"
    assert n("(k_open_uniform<ST_REGION, false>)") == n("(k_open_uniform<ST_REGION, false, 16>)") == "k_open_uniform<2,false,16>"
    assert n("(k_open_uniform<ST_SHIFT, true, 8>)") == "k_open_uniform<3,true,8>"
    assert n("(k_seal_uniform_ina<ST_SHIFT, true, 1>)") == "k_seal_uniform_ina<3,true,1>"
    assert n("(k_open_uniform_carry<8>)") == "k_open_uniform_carry<8>" and n("k_zero_pad") == "k_zero_pad"


def test_golden_covers_every_instantiation():
    """The case grid reaches every branch of every launcher: the kernels in the parent's record are
    exactly the launchers' instantiation sets."""
    got = dispatch_record.signatures(open(GOLDEN).read())
    assert got == INSTANTIATIONS, (sorted(got - INSTANTIATIONS), sorted(INSTANTIATIONS - got))


@needs_hipcc
def test_working_tree_dispatches_as_the_parent():
    want = open(GOLDEN).read()
    got = dispatch_record.record()
    if got != want:
        w, g = want.splitlines(), got.splitlines()
        first = next((i for i, (a, b) in enumerate(zip(w, g)) if a != b), min(len(w), len(g)))
        case = next((ln for ln in reversed(w[:first + 1]) if not ln.startswith(" ")), "")
        pytest.fail(f"dispatch differs from the parent's at line {first + 1} (case {case!r}):\n"
                    f"  parent: {w[first] if first < len(w) else '<end>'}\n  tree:   {g[first] if first < len(g) else '<end>'}")
