"""The four fused launches of csrc/ff_fused.hip (ff_fused_kernel, ff_proj_fused_kernel, ff_proj_fused_h16_kernel, l0_head_kernel)
against the output BITS recorded in tests/golden/ff_fused_bits.json (tests/golden/make_golden_ff_fused.py: the cases, and why these).

The other tests of these kernels compare them with the launches they replace, within bounds that would not notice a changed order
of an fp32 sum.  This one holds a refactor of the file to "nothing changed": per case the sha256 of every output tensor must equal the
recorded one, and the call must have been exactly one launch (no quiet route through the separate launches).  A change that really
alters a summation order regenerates the fixture (python tests/golden/make_golden_ff_fused.py on the device) and says so in its
description; a mismatch here is otherwise a bug.  If the INPUT hash differs, the generator or the random stream drifted and the
comparison means nothing: that fails too, it does not skip."""
import json
import sys
from pathlib import Path

import pytest

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
import make_golden_ff_fused as mk  # noqa: E402


@pytest.fixture(scope="module")
def recorded():
    return json.loads(mk.OUT.read_text())["cases"]


def test_fixture_lists_every_case():
    assert sorted(json.loads(mk.OUT.read_text())["cases"]) == sorted(mk.CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(mk.CASES))
def test_output_bits(name, recorded):
    got, launches = mk.run_case(name)
    want = recorded[name]
    print(f"{name}: {launches} launch(es), outputs {got['outputs']}")
    assert launches == 1, f"{name} took {launches} launches: the fused kernel was not used"
    assert got["inputs"] == want["inputs"], (f"{name}: the generated inputs are not the recorded ones -- "
                                             "tests/golden/make_golden_ff_fused.py (or torch's random stream) drifted from the fixture")
    assert sorted(got["outputs"]) == sorted(want["outputs"])
    for k, v in got["outputs"].items():
        assert v == want["outputs"][k], f"{name}: the bits of `{k}` differ from tests/golden/ff_fused_bits.json"
