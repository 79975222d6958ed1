"""CPU: the GEMM / convolution tile selection (csrc/gemm_select.h) against tests/golden/gemm_select_table.txt.

Every tile walks K in the same order, so a tile that is wrong for a shape still gives the right numbers and no GPU test notices; this
table does.  tests/gemm_select_probe.cpp is compiled with the host compiler (the header is plain C++) and run over the table's inputs.
An intentional retune regenerates the expected column (tests/golden/make_golden_gemm_select.py --write) and shows up as a diff."""
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
sys.path.insert(0, str(GOLDEN))
import make_golden_gemm_select as grid  # noqa: E402

# every id launch_by_id (csrc/gemm.hip) knows, per kernel family
CONV_IDS = {1, 2, 3, 4, 13, 20, 21, 22, 23, 24, 31, 32, 33, 34, 35, 36, 37, 46}
GEMM_IDS = {1, 2, 3, 4, 14, 21, 22, 23, 24, 46, 61, 63, 64, 65, 67, 69}


@pytest.fixture(scope="module")
def table():
    rows = [l.split(" | ") for l in grid.TABLE.read_text().splitlines() if l and not l.startswith("#")]
    assert all(len(r) == 2 for r in rows)
    return rows


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("gemm_select") / "gemm_select_probe"
    # the header must need nothing from HIP: the host compiler alone, the two include directories of the build
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", f"-I{ROOT / 'include'}", f"-I{ROOT / 'diffuman4d_amd' / 'csrc'}",
                    str(grid.PROBE_SRC), "-o", str(exe)], check=True)
    return exe


def test_table_inputs_are_the_generators(table):
    assert [r[0] for r in table] == grid.inputs()


def test_selection_matches_table(table, probe):
    got = grid.run_probe([r[0] for r in table], exe=probe)
    want = [" | ".join(r) for r in table]
    assert len(got) == len(want)
    diff = [(w, g) for w, g in zip(want, got) if w != g]
    assert not diff, f"{len(diff)} of {len(want)} shapes changed their configuration (expected, got), first ones: {diff[:8]}"


def _choices(table, kind):
    """(column, id, splits) of every choice in the rows of `kind`; the workspace column of a convolution row is skipped"""
    for inp, exp in table:
        if inp[0] != kind:
            continue
        for col, cell in enumerate(exp.split()):
            if (kind == "c" and col == 2) or cell == "unsupported":
                continue
            i, s = cell.split("/")
            yield col, int(i), int(s)


def test_grid_reaches_every_configuration(table):
    """A grid that stops reaching a branch of the heuristic would pass quietly: every id must be chosen somewhere."""
    assert {i for _, i, _ in _choices(table, "c")} == CONV_IDS
    assert {i for _, i, _ in _choices(table, "g")} == GEMM_IDS
    assert {exp for inp, exp in table if inp[0] == "u"} == {"256x128", "128x128", "128x64"}
    assert any("unsupported" in exp for _, exp in table)


def test_grid_has_the_split_rows(table):
    """Convolution columns: fast, fast_ws, ws_bytes, par_ws, f16, f16_ws.  Only a launch with a workspace splits, and always as id 31 x 3;
    the parity precision never does."""
    by_col = {}
    for col, i, s in _choices(table, "c"):
        assert s in (1, 3) and (s == 1 or i == 31)
        by_col.setdefault(col, set()).add(s)
    assert by_col[0] == {1} and by_col[3] == {1} and by_col[4] == {1}
    assert by_col[1] == {1, 3} and by_col[5] == {1, 3}
    for inp, exp in table:
        if inp[0] == "c":
            e = exp.split()
            assert e[1].endswith("/3") == e[5].endswith("/3") and (int(e[2]) > 0 or not e[1].endswith("/3"))
    assert all(s == 1 for _, _, s in _choices(table, "g"))
