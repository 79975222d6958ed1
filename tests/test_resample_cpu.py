"""CPU: host/resample.py -- the one table packer (TableSet) against what SpaTemDataset._tables returned before the packers were joined
(tests/golden/resample_tableset.npz: that method's tables and int32 array for one seeded task of seven crops at 48 x 64, whose size
pairs repeat, swap, scale up and down and include the identity), and the import order of the modules that share it."""
import itertools
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from diffuman4d_amd.host import capture, resample

ROOT = Path(__file__).resolve().parent.parent
REF = np.load(ROOT / "tests" / "golden" / "resample_tableset.npz")


def test_table_set_packs_as_the_dataset_did():
    H, W = int(REF["height"]), int(REF["width"])
    ts = resample.TableSet()
    for _, _, ch, cw in REF["crops"].tolist():
        h_at, v_at = ts.add(cw, W), ts.add(ch, H)
        assert ts.add(cw, W) == h_at and ts.add(ch, H) == v_at  # a pair seen before keeps its place and adds nothing
    assert list(ts.tables) == [tuple(p) for p in REF["pairs"].tolist()]
    assert list(ts.tables.values()) == [tuple(v) for v in REF["where"].tolist()]
    tab = ts.array()
    assert tab.dtype == np.int32 and np.array_equal(tab, REF["tab"])
    for (n_in, n_out), (off, ksize) in ts.tables.items():  # every table lies where its offset says
        b, k = resample.bicubic_table(n_in, n_out)
        assert k.shape[1] == ksize
        assert np.array_equal(tab[off: off + b.size + k.size], np.concatenate([b.reshape(-1), k.reshape(-1)]))


def test_the_dataset_uses_the_table_set():
    ds = capture.SpaTemDataset.__new__(capture.SpaTemDataset)
    ds.height, ds.width = int(REF["height"]), int(REF["width"])
    tables, tab = ds._tables([{"crop": tuple(c)} for c in REF["crops"].tolist()])
    assert list(tables.items()) == [(tuple(p), tuple(v)) for p, v in zip(REF["pairs"].tolist(), REF["where"].tolist())]
    assert tab.dtype == np.int32 and np.array_equal(tab, REF["tab"])


def test_capture_re_exports_the_one_definition():
    assert capture.bicubic_table is resample.bicubic_table and capture.PRECISION_BITS == resample.PRECISION_BITS == 22


@pytest.mark.parametrize("order", list(itertools.permutations(("skeleton", "jpeg", "capture"))), ids="-".join)
def test_modules_import_in_any_order(order):
    code = "; ".join(f"import diffuman4d_amd.host.{m}" for m in order) + "; print('ok')"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(ROOT))
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]
