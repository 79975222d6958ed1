"""CPU: the cell cache of SpaTemDataset(device_cache=True).  CellCache (host/capture_cache.py) launches nothing: its state machine,
budget, slab growth and claim protocol are tested on a CPU device, two threads stepped with barriers and events.  The dataset's route runs
against a flag-off dataset with the two new device entries replaced by their numpy stand-ins (tests/capture_cache_standin.py)."""
import shutil
import threading

import numpy as np
import pytest
import torch
from PIL import Image

import capture_cache_standin as cs
import capture_model as cm
import kp2d_scene as ks
from diffuman4d_amd.host import capture, skeleton
from diffuman4d_amd.host.capture_cache import Cell, CellCache

CB = 64  # a cell of 8 pixels


def fill(cache, keys):
    """claim, reserve and publish `keys` -> the reservations."""
    hits, owned, others = cache.claim(keys)
    assert not hits and not others and owned == list(keys)
    slots = cache.reserve(owned)
    for k, s in zip(owned, slots):
        if s is None:
            cache.abandon([k])
        else:
            cache.publish(k, ("crop", k))
    return slots


# -- CellCache ------------------------------------------------------------------------------------------------------------------------
def test_state_machine():
    c = CellCache("cpu", CB, 1 << 20, slab_cells=4)
    assert c.state("a") == "absent" and c.stats == {"hits": 0, "misses": 0, "unretained": 0, "cells": 0, "bytes": 0}
    hits, owned, others = c.claim(["a", "b", "a"])
    assert (hits, owned, others) == ([], ["a", "b"], []) and c.state("a") == c.state("b") == "pending"
    assert c.claim(["b", "c"]) == ([], ["c"], ["b"])  # pending elsewhere: not ours, no hit
    (slab, off), (slab_b, off_b) = c.reserve(["a", "b"])
    assert slab is slab_b and slab.dtype == torch.uint8 and slab.numel() == 4 * CB and {off, off_b} == {0, CB} and slab.data_ptr() % 16 == 0
    c.publish("a", [1, 2, 3])
    assert c.state("a") == "ready" and c.state("b") == "pending"
    hits, owned, others = c.claim(["a", "b"])
    assert owned == [] and others == ["b"] and hits == [Cell("a", slab, off, [1, 2, 3], None)] and hits[0].slab is slab
    c.abandon(["b", "c", "a"])  # "a" is ready: left alone
    assert c.state("b") == c.state("c") == "absent" and c.state("a") == "ready"
    assert c.claim(["b"]) == ([], ["b"], [])  # an abandoned key can be claimed again, and gets the cell that was given back
    assert c.reserve(["b"]) == [(slab, off_b)]
    c.publish("b", None)
    assert c.stats == {"hits": 1, "misses": 4, "unretained": 0, "cells": 2, "bytes": 4 * CB}
    for bad in (lambda: c.publish("zz", None), lambda: c.publish("a", None), lambda: c.reserve(["a"]), lambda: c.reserve(["nobody"])):
        with pytest.raises(RuntimeError):
            bad()
    for kw in ({"cell_bytes": 0}, {"cell_bytes": 24}, {"budget_bytes": -1}, {"slab_cells": 0}):
        with pytest.raises(ValueError):
            CellCache("cpu", **{"cell_bytes": CB, "budget_bytes": 0, **kw})


@pytest.mark.parametrize("budget_cells,slab_cells,kept", [(0, 4, 0), (3, 4, 0), (4, 4, 4), (5, 2, 4), (7, 4, 4), (8, 4, 8), (100, 4, 10)])
def test_the_budget_is_never_exceeded_and_slabs_grow_on_demand(budget_cells, slab_cells, kept):
    c = CellCache("cpu", CB, budget_cells * CB, slab_cells=slab_cells)
    seen = []
    for k in range(10):
        (slot,) = fill(c, [k])
        assert c.stats["bytes"] <= budget_cells * CB
        assert c.stats["bytes"] == -(-min(k + 1, kept) // slab_cells) * slab_cells * CB  # a slab appears when its first cell is asked for
        assert (slot is None) == (k >= kept) and c.state(k) == ("ready" if k < kept else "absent")
        if slot is not None:
            seen.append((slot[0].data_ptr(), slot[1]))
    assert len(set(seen)) == kept and c.stats["cells"] == kept and c.stats["unretained"] == 10 - kept and c.stats["misses"] == 10
    hits, owned, _ = c.claim(range(10))
    assert [h.key for h in hits] == list(range(kept)) and owned == list(range(kept, 10))  # what was not retained is simply loaded again


def test_clear():
    c = CellCache("cpu", CB, 8 * CB, slab_cells=4)
    fill(c, ["a", "b", "c", "d", "e"])
    assert c.stats["cells"] == 5 and c.stats["bytes"] == 8 * CB
    c.clear()
    assert c.stats == {"hits": 0, "misses": 5, "unretained": 0, "cells": 0, "bytes": 0} and c.state("a") == "absent"
    fill(c, ["a"])
    assert c.stats["cells"] == 1 and c.stats["bytes"] == 4 * CB
    c.claim(["z"])
    with pytest.raises(RuntimeError, match="pending"):
        c.clear()


def test_two_threads_share_out_overlapping_keys_and_wait_for_each_other():
    """Thread A asks for 0..5, thread B for 3..8, both at a barrier.  Whatever the interleaving: each key has one owner, each thread
    publishes what it owns before it waits for the other's keys, and both end with all their cells."""
    c = CellCache("cpu", CB, 1 << 20, slab_cells=4)
    start = threading.Barrier(2)
    owners, result, errors = {}, {}, []

    def run(name, keys):
        try:
            start.wait(timeout=30)
            hits, owned, others = c.claim(keys)
            owners[name] = owned
            for k, (slab, off) in zip(owned, c.reserve(owned)):
                c.publish(k, name)
            c.wait(others)
            more, owned2, others2 = c.claim(others)
            assert not owned2 and not others2
            result[name] = {h.key: h.meta for h in hits + more}
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    ts = [threading.Thread(target=run, args=("A", list(range(6))), daemon=True), threading.Thread(target=run, args=("B", list(range(3, 9))), daemon=True)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=30)
    assert not errors and not any(t.is_alive() for t in ts)
    assert sorted(owners["A"] + owners["B"]) == list(range(9)) and set(owners["A"]) >= {0, 1, 2} and set(owners["B"]) >= {6, 7, 8}
    assert all(result["A"][k] == "B" for k in set(range(3, 6)) & set(owners["B"]))
    assert all(result["B"][k] == "A" for k in set(range(3, 6)) & set(owners["A"]))
    assert c.stats["misses"] == 9 and c.stats["cells"] == 9


def test_each_thread_waits_for_the_others_keys_without_deadlock_and_an_abandoned_key_comes_back():
    """A owns {a1, x}, B owns {b1, y}; A also wants y, B also wants x.  The claims are stepped so that both hold pending keys the other
    wants; A abandons x (its load failed), B publishes y.  Neither waits before it has settled what it owns: no deadlock; B finds x
    absent after the wait and claims it."""
    c = CellCache("cpu", CB, 1 << 20, slab_cells=4)
    a_claimed, b_claimed, a_saw_y = threading.Event(), threading.Event(), threading.Event()
    out, errors = {}, []

    def thread_a():
        try:
            assert c.claim(["a1", "x"]) == ([], ["a1", "x"], [])
            a_claimed.set()
            assert b_claimed.wait(timeout=30)
            hits, owned, others = c.claim(["y"])
            assert (hits, owned, others) == ([], [], ["y"])
            a_saw_y.set()
            c.reserve(["a1", "x"])
            c.abandon(["a1", "x"])  # the load raised: nothing published
            c.wait(others)
            out["A"] = c.claim(others)
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    def thread_b():
        try:
            assert a_claimed.wait(timeout=30)
            assert c.claim(["b1", "y", "x"]) == ([], ["b1", "y"], ["x"])
            b_claimed.set()
            assert a_saw_y.wait(timeout=30)
            c.reserve(["b1", "y"])
            c.publish("b1", "B")
            c.publish("y", "B")
            c.wait(["x"])
            out["B"] = c.claim(["x"])
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    ts = [threading.Thread(target=thread_a, daemon=True), threading.Thread(target=thread_b, daemon=True)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=30)
    assert not errors and not any(t.is_alive() for t in ts)
    hits, owned, others = out["A"]
    assert [h.key for h in hits] == ["y"] and hits[0].meta == "B" and not owned and not others
    assert out["B"] == ([], ["x"], [])  # abandoned by A: absent again, B owns it now
    assert c.state("a1") == "absent" and c.state("x") == "pending" and c.stats["cells"] == 2


# -- the stand-ins are the definition, in the cell format ---------------------------------------------------------------------------------
def test_the_stand_ins_round_trip_equals_the_fused_model():
    rng = np.random.default_rng(5)
    H, W, sizes = 5, 8, [(37, 53), (9, 5)]
    crops = [(-3, -4, 30, 40), (2, 1, 4, 3)]
    ts = capture.TableSet()
    planes, offs, cur = [], [], 0
    for (h, w), (top, left, ch, cw) in zip(sizes, crops):
        ts.add(cw, W), ts.add(ch, H)
        fr = []
        for c in (3, 1, 3):
            planes.append(rng.integers(0, 256, h * w * c, dtype=np.uint8))
            fr.append(cur)
            cur += h * w * c
        offs.append(fr)
    tab = ts.array()
    desc = np.zeros((2, capture.FIELDS), np.int64)
    for f, ((h, w), (top, left, ch, cw)) in enumerate(zip(sizes, crops)):
        desc[f, :9] = [*offs[f], h, w, top, left, ch, cw]
    blob = torch.from_numpy(np.concatenate(planes + [np.zeros(-cur % 8, np.uint8), desc.view(np.uint8).reshape(-1)]))
    desc_off = cur + (-cur % 8)
    slab = torch.full((3 * H * W * 8 + 32,), 0xA5, dtype=torch.uint8)
    cells = torch.tensor([[slab.data_ptr(), slab.numel(), 2 * H * W * 8 + 32, 0], [slab.data_ptr(), slab.numel(), 16, 0]], dtype=torch.int64)
    cs.standin_crop_resize_packed(blob, blob, 2, desc_off, 0, 1, H, W, cells, cells.clone())
    s = slab.numpy()
    assert (s[:16] == 0xA5).all() and (s[16 + H * W * 8: 2 * H * W * 8 + 32] == 0xA5).all()
    cells[:, 3] = torch.tensor([2, 0])
    pix, skel = cs.standin_unpack_cells(cells, cells.clone(), 3, H, W, out=(torch.full((3, 3, H, W), 7.0), torch.full((3, 3, H, W), 7.0)))
    want_pix, want_skel = cm.standin_crop_resize(blob, blob, 2, desc_off, 0, 1, H, W)
    assert torch.equal(pix[2], want_pix[0]) and torch.equal(pix[0], want_pix[1]) and torch.equal(skel[2], want_skel[0]) and torch.equal(skel[0], want_skel[1])
    assert (pix[1] == 7.0).all() and (skel[1] == 7.0).all()


# -- the dataset on stand-ins ---------------------------------------------------------------------------------------------------------
PALETTE = skeleton.load_palette(ks.PALETTE_PATH)
HW = ks.SIZES[0]
OUT = 64


def cheap_maps(plans):
    """Skeleton files for the files route: any non-empty RGB map does, one colour per file."""
    h, w = HW
    maps = np.zeros((len(plans), h, w, 3), np.uint8)
    for k, m in enumerate(maps):
        m[h // 4 + k: 3 * h // 4, w // 3: 2 * w // 3 + k] = (40 + 10 * k, 255 - 9 * k, 17 * k % 256)
    return maps


@pytest.fixture(scope="module")
def scene_root(tmp_path_factory):
    root = tmp_path_factory.mktemp("cache_cpu")
    scene = ks.write_cameras_and_detections(root, HW)
    ks.detections_as_poses_2d(scene)
    ks.write_images_and_masks(scene, HW)
    ks.write_skeleton_pngs(scene, HW, PALETTE, cheap_maps)
    return root


@pytest.fixture
def standins(monkeypatch):
    calls = {"fused": 0, "packed": 0, "unpack": 0}

    def count(name, fn):
        def w(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        return w
    monkeypatch.setattr(capture.ops, "capture_crop_resize", count("fused", cm.standin_crop_resize))
    monkeypatch.setattr(capture.ops, "capture_crop_resize_packed", count("packed", cs.standin_crop_resize_packed))
    monkeypatch.setattr(capture.ops, "capture_unpack_cells", count("unpack", cs.standin_unpack_cells))
    return calls


def dataset(root, **kw):
    return capture.SpaTemDataset(data_dir=str(root), scene_label=ks.SCENE, device="cpu", decode_threads=4, height=OUT, width=OUT,
                                 **{**ks.patterns(), **kw})


def keys_of(labels, inputs=ks.INPUTS):
    return [(None, scene, spa, tem, spa in inputs) for scene, spa, tem in labels]


@pytest.mark.parametrize("has_gt_target", [True, False])
def test_the_sequence_equals_flag_off_and_calls_3_and_4_open_no_file(scene_root, standins, monkeypatch, has_gt_target):
    opened = cs.OpenLog(monkeypatch)
    off, on = dataset(scene_root, has_gt_target=has_gt_target), dataset(scene_root, has_gt_target=has_gt_target, device_cache=True)
    assert off.device_cache is False and off.cache_stats == {"hits": 0, "misses": 0, "unretained": 0, "cells": 0, "bytes": 0}
    opened_by_call = {}
    for call, (spa, tem) in enumerate(cs.sequence(ks), 1):
        want = off.get_item(ks.SCENE, spa, tem, ks.INPUTS)
        files_off = opened.take()
        got = on.get_item(ks.SCENE, spa, tem, ks.INPUTS)
        files_on = opened.take()
        cs.same(got, want)
        assert all(a is not b for a, b in zip(got["crops"], on.get_item(ks.SCENE, spa, tem, ks.INPUTS)["crops"]))  # the cache's lists are not handed out
        assert opened.take() == []  # and that repeat opened nothing
        assert files_off and files_on == (files_off if call <= 2 else []), call
        opened_by_call[call] = files_off
    assert standins == {"fused": 4, "packed": 2, "unpack": 8}
    assert on.cache_stats == {"hits": 16 + 4 + 4 + 8 + 8, "misses": 16, "unretained": 0, "cells": 16, "bytes": 64 * OUT * OUT * 8}
    on.clear_device_cache()
    assert on.cache_stats["cells"] == 0 and on.cache_stats["bytes"] == 0
    got = on.get_item(ks.SCENE, *cs.sequence(ks)[2], ks.INPUTS)  # a cleared cache loads again: exactly what flag off opens for call 3
    assert opened.take() == opened_by_call[3]
    cs.same(got, off.get_item(ks.SCENE, *cs.sequence(ks)[2], ks.INPUTS))


def test_a_budget_of_five_cells(scene_root, standins):
    off = dataset(scene_root)
    on = dataset(scene_root, device_cache=True, device_cache_bytes=5 * OUT * OUT * 8)
    for spa, tem in cs.sequence(ks):
        cs.same(on.get_item(ks.SCENE, spa, tem, ks.INPUTS), off.get_item(ks.SCENE, spa, tem, ks.INPUTS))
        st = on.cache_stats
        assert st["cells"] <= 5 and st["bytes"] <= 5 * OUT * OUT * 8
    assert st["unretained"] > 0 and st["unretained"] == st["misses"] - st["cells"]


def test_a_truncated_mask_raises_the_same_and_leaves_the_calls_cells_absent(scene_root, standins, tmp_path):
    shutil.copytree(scene_root / ks.SCENE, tmp_path / ks.SCENE)
    mask = tmp_path / ks.SCENE / "fmasks" / "04" / f"{ks.FRAMES[1]}.png"
    whole = mask.read_bytes()
    mask.write_bytes(whole[: len(whole) // 2])
    off, on = dataset(tmp_path), dataset(tmp_path, device_cache=True)
    (spa0, tem0), (spa1, tem1) = cs.sequence(ks)[:2]
    cs.same(on.get_item(ks.SCENE, spa0, tem0, ks.INPUTS), off.get_item(ks.SCENE, spa0, tem0, ks.INPUTS))
    errors = []
    for ds in (off, on):
        with pytest.raises(Exception) as e:
            ds.get_item(ks.SCENE, spa1, tem1, ks.INPUTS)
        errors.append((type(e.value), str(e.value)))
    assert errors[0] == errors[1]
    cache = on._cache(torch.device("cpu"))
    assert all(cache.state(k) == "absent" for k in keys_of([(ks.SCENE, s, tem1[0]) for s in spa1]))
    assert all(cache.state(k) == "ready" for k in keys_of([(ks.SCENE, s, tem0[0]) for s in spa0]))
    assert on.cache_stats["cells"] == 8 and on.cache_stats["misses"] == 16
    mask.write_bytes(whole)
    cs.same(on.get_item(ks.SCENE, spa1, tem1, ks.INPUTS), off.get_item(ks.SCENE, spa1, tem1, ks.INPUTS))
    assert on.cache_stats["cells"] == 16 and on.cache_stats["misses"] == 24


def test_the_key_tells_an_input_camera_from_a_target(scene_root, standins):
    """has_gt_target=False: camera 03 as a target is its skeleton's box; as an input camera it is its image.  Two cells."""
    on, off = dataset(scene_root, has_gt_target=False, device_cache=True), dataset(scene_root, has_gt_target=False)
    spa, tem = cs.sequence(ks)[0]
    for inputs in (ks.INPUTS, ["01", "03"], ks.INPUTS):
        cs.same(on.get_item(ks.SCENE, spa, tem, inputs), off.get_item(ks.SCENE, spa, tem, inputs))
    assert on.cache_stats["cells"] == 8 + 2  # cameras 03 and 05 changed sides once


def test_the_data_config_takes_the_two_keys_and_selects_the_native_class():
    from diffuman4d_amd.host import config
    assert config.NATIVE_DATASET_KEYS["device_cache"] is False and config.NATIVE_DATASET_KEYS["device_cache_gb"] == 16
    base = ["exp=demo_3d", f"data.data_dir={ks.GOLDEN / 'triang_scene'}", f"data.scene_label={ks.SCENE}", "data.height=64", "data.width=64"]
    ds = config.instantiate(config.compose(base + ["data.device_cache=true", "data.device_cache_gb=2"])["data"])
    assert type(ds) is capture.SpaTemDataset and ds.device_cache is True and ds.device_cache_bytes == 2 << 30
    ds = config.instantiate(config.compose(base + ["data.device_cache=true"])["data"])
    assert type(ds) is capture.SpaTemDataset and ds.device_cache is True and ds.device_cache_bytes == 16 << 30
    ds = config.instantiate(config.compose(base + ["data.device_cache_gb=0.5", "data.device_cache=true"])["data"])
    assert ds.device_cache_bytes == 1 << 29
    import inspect
    p = inspect.signature(capture.SpaTemDataset.__init__).parameters
    assert p["device_cache"].default is False and p["device_cache_bytes"].default == 16 << 30
