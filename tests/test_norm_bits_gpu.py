"""Every kernel of csrc/norm.hip (GroupNorm single-launch / two-launch / fp64 general, LayerNorm, the three row softmaxes) against the
output BITS recorded in tests/golden/norm_bits.json (tests/golden/make_golden_norm.py: the cases, and why these).

The opcheck cases of these kernels compare them with fp64 references, within bounds that would not notice a changed order of a sum.
This one holds a refactor of the file to "nothing changed": per case the sha256 of every output tensor must equal the recorded one.
A change that really alters a summation order regenerates the fixture (python tests/golden/make_golden_norm.py on the device) and
says so in its description; a mismatch here is otherwise a bug.  If the INPUT hash differs, the generator or the random stream
drifted and the comparison means nothing: that fails too, it does not skip."""
import json
import sys
from pathlib import Path

import pytest

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
import make_golden_norm as mk  # noqa: E402


@pytest.fixture(scope="module")
def recorded():
    return json.loads(mk.OUT.read_text())["cases"]


def test_fixture_lists_every_case():
    assert sorted(json.loads(mk.OUT.read_text())["cases"]) == sorted(mk.CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(mk.CASES))
def test_output_bits(name, recorded):
    got = mk.run_case(name)
    want = recorded[name]
    print(f"{name}: outputs {got['outputs']}")
    assert got["inputs"] == want["inputs"], (f"{name}: the generated inputs are not the recorded ones -- "
                                             "tests/golden/make_golden_norm.py (or torch's random stream) drifted from the fixture")
    assert sorted(got["outputs"]) == sorted(want["outputs"])
    for k, v in got["outputs"].items():
        assert v == want["outputs"][k], f"{name}: the bits of `{k}` differ from tests/golden/norm_bits.json"
