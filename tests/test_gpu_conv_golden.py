"""The direct and the fp32 Winograd convolutions, bit for bit: sha256 of the output bytes of every case of
tools/gen_conv_golden.py against tests/golden/conv_golden.json (generated once, through entry points that did not change
since, on the library as it was before the profiling hooks and ablation masks left these kernels).  The other tests of
these kernels compare with a tolerance; a digest sees a changed summation order, a skipped stage or a lost store.

Tolerance: none.  The kernels are deterministic (fixed summation order, no atomics) and the inputs are seeded host arrays."""
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_conv_golden", os.path.join(ROOT, "tools", "gen_conv_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


@pytest.fixture(scope="module")
def digests():
    with open(G.GOLDEN) as f:
        return json.load(f)


def test_every_case_has_a_digest(digests):
    assert sorted(digests) == sorted(G.case_id(c) for c in G.CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_conv_output_bits(case, dev, digests):
    out = G.run_case(case, dev)
    assert np.isfinite(out).all(), "an output element was not written"
    print(G.case_id(case), G.kernel_of(case), G.digest(out))
    assert G.digest(out) == digests[G.case_id(case)], f"{G.kernel_of(case)}: output bits differ from tests/golden/conv_golden.json"
