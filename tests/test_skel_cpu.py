"""CPU: the host half of skeleton-map drawing (diffuman4d_amd/host/skeleton.py) against the reference's recorded draw calls
(tests/golden/skel_reference.json, written by tests/golden/make_golden_skel.py from the reference's own draw_one_skeleton with a
recording cv2), the numpy model of the rasteriser (tests/skel_model.py) on a case computed by hand, and the argument checks that
dm4d_skeleton_draw_u8 makes on its host copies before it launches anything."""
import ctypes
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import skel_model
from diffuman4d_amd.host import lib as L, ops, skeleton
from diffuman4d_amd.host.capture import bicubic_table

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
PALETTE_PATH = GOLDEN / "skel_palette.json"
CASES = {c["name"]: c for c in json.loads((GOLDEN / "skel_reference.json").read_text())["cases"]}
PALETTE = skeleton.load_palette(PALETTE_PATH)


def plan(case, **kw):
    return skeleton.plan_draw_calls(case["instance"], case["score_instance"], (case["kp2d_canvas_shape"], case["out_kpmap_shape"]), PALETTE, **kw)


def in_range(call):
    pts = [call["p1"], call["p2"]] if call["type"] == "line" else [call["center"]]
    return all(skeleton.COORD_MIN <= v <= skeleton.COORD_MAX for p in pts for v in p)


def recorded_calls(case):
    """The reference's calls, without the links (line, circle, circle) that have an endpoint outside [-8192, 8191] -> (calls, dropped)."""
    groups = [case["calls"][i:i + 3] for i in range(0, len(case["calls"]), 3)]
    assert all([c["type"] for c in g] == ["line", "circle", "circle"] for g in groups)
    kept = [g for g in groups if in_range(g[0])]
    return [c for g in kept for c in g], len(groups) - len(kept)


@pytest.mark.parametrize("name", list(CASES))
def test_plan_is_the_reference_s_call_list(name):
    case = CASES[name]
    got = plan(case)
    want, dropped = recorded_calls(case)
    assert got.canvas_shape == tuple(case["canvas_shape"])
    assert list(got.out_size) == case["saved_size"]
    assert got.dropped_links == dropped and (dropped > 0) == (name == "off_canvas_beyond_range")
    assert len(got.calls) == len(want)
    for k, (a, b) in enumerate(zip(got.calls, want)):
        assert a == b, (name, k, a, b)


def test_the_fixture_covers_what_it_says():
    by = CASES
    assert by["shape_1000x600"]["saved_size"] == [599, 1000] and by["shape_2500x1500"]["canvas_shape"] == [2048, 1228]
    assert len(by["ones_no_depths"]["calls"]) == 3 * 67 and "keypoint_scores" not in by["ones_no_depths"]["instance"]
    assert "keypoint_depths" in by["depths_with_a_tie"]["instance"]
    lines = [c for c in by["hands_in_one_tile"]["calls"] if c["type"] == "line"]
    hand = [c for c in lines if all(576 <= v < 640 for v in c["p1"] + c["p2"])]  # canvas pixels of the output tile 288 .. 319
    assert len(hand) >= 40 and sum(c["p1"] == c["p2"] for c in hand) == 2
    off = [c for c in by["off_canvas_inside_range"]["calls"] if c["type"] == "line" and max(c["p1"] + c["p2"]) > 2048]
    assert off and max(max(c["p1"] + c["p2"]) for c in off) == 8191
    # ties: an even and an odd k + 0.5 both occur among the doubled keypoints
    kp = np.array(by["rounding_ties"]["instance"]["keypoints"], dtype=np.float32)[:23] * 2
    frac_half = kp[np.abs(kp - np.floor(kp) - 0.5) < 1e-6]
    assert (np.floor(frac_half) % 2 == 0).any() and (np.floor(frac_half) % 2 == 1).any()


def test_sort_branches_and_thresholds():
    tie = plan(CASES["depths_with_a_tie"]).calls
    depth = np.array(CASES["depths_with_a_tie"]["instance"]["keypoint_depths"], dtype=np.float32)
    links = {tuple(l["link"]): l["id"] for l in PALETTE.links}
    # the two links of equal mean depth (ids 8 and 9) are painted next to each other, in the palette's order
    kp = np.array(CASES["depths_with_a_tie"]["instance"]["keypoints"], dtype=np.float32) * 2
    pos = {}
    for k, c in enumerate(tie[::3]):
        for (a, b), lid in links.items():
            if lid in (8, 9) and c["p1"] == [int(round(float(kp[a][0]))), int(round(float(kp[a][1])))] and \
                    c["p2"] == [int(round(float(kp[b][0]))), int(round(float(kp[b][1])))]:
                pos[lid] = k
    assert pos[8] + 1 == pos[9]
    assert float(depth[5] + depth[7]) == float(depth[6] + depth[8])
    # thresholds: a score of exactly 0.5 is drawn (black), one just below is not; 0.9 and above give the full colour
    inst = CASES["thresholds_and_negative_coordinates"]["instance"]
    calls = plan(CASES["thresholds_and_negative_coordinates"]).calls
    p15 = [int(round(v * 2)) for v in inst["keypoints"][15]]
    p16 = [int(round(v * 2)) for v in inst["keypoints"][16]]
    assert any(c["type"] == "line" and c["p1"] == p15 and c["color"] == [0, 0, 0] for c in calls)
    assert not any(c["type"] == "line" and p16 in (c["p1"], c["p2"]) for c in calls)
    assert not any(c["type"] == "circle" and min(c["center"]) < 0 for c in calls)


def test_error_cases():
    case = CASES["scores_only"]
    with pytest.raises(NotImplementedError):
        plan(case, draw_face_keypoints=True)
    short = skeleton.Palette(PALETTE.keypoint_colors[:-1], [l for l in PALETTE.links if max(l["link"]) < 132], PALETTE.x_link_color)
    with pytest.raises(ValueError, match=r"the length of kpt_color \(132\)"):
        skeleton.plan_draw_calls(case["instance"], None, ((1024, 1024), (1024, 1024)), short)
    with pytest.raises(ValueError, match="thickness rounds to 0"):
        skeleton.plan_draw_calls(case["instance"], None, ((16384, 16384), (1024, 1024)), PALETTE)
    for shape in ((255, 255), (128, 64), (8193, 100)):
        with pytest.raises(ValueError, match="256 .. 8192"):
            skeleton.draw_skeleton_maps([], None, out_kpmap_shape=shape, palette=PALETTE)


def test_palette_loading(tmp_path):
    data = json.loads(PALETTE_PATH.read_text())
    assert len(PALETTE.keypoint_colors) == 133 and [l["id"] for l in PALETTE.links] == list(range(65))
    with pytest.raises(ValueError, match="no palette given.*classes_and_palettes"):
        skeleton.load_palette(None)
    with pytest.raises(FileNotFoundError, match="COCO_WHOLEBODY_KPTS_COLORS"):
        skeleton.load_palette(tmp_path / "absent.json")
    bad = dict(data, keypoint_colors=data["keypoint_colors"][:100])  # the hand links now point past the colours
    with pytest.raises(ValueError, match="there are 100 keypoint colours"):
        skeleton.make_palette(bad)
    bad = dict(data, x_link_color=[1, 2])
    with pytest.raises(ValueError, match="x_link_color"):
        skeleton.make_palette(bad)
    bad = dict(data, links=data["links"] + [data["links"][3]])
    with pytest.raises(ValueError, match="used twice"):
        skeleton.make_palette(bad)
    with pytest.raises(ValueError, match="expected the keys"):
        skeleton.make_palette({"links": []})
    p = tmp_path / "p.json"
    p.write_text(json.dumps(data))
    assert skeleton.load_palette(str(p)) == PALETTE
    # nothing in the package holds a table of its own
    src = (ROOT / "diffuman4d_amd" / "host" / "skeleton.py").read_text()
    assert "[116, 192, 252]" not in src and "116, 192, 252" not in src


def test_out_of_range_link_is_dropped_and_counted():
    case = CASES["off_canvas_beyond_range"]
    got = plan(case)
    touching = [l["id"] for l in PALETTE.links if 16 in l["link"] or 9 in l["link"]]  # the two keypoints the case moves out of range
    assert touching == [2, 10, 22, 23, 24]
    assert got.dropped_links == 5 and len(got.calls) == len(case["calls"]) - 15
    assert all(in_range(c) for c in got.calls)
    assert plan(CASES["off_canvas_inside_range"]).dropped_links == 0


def test_model_paints_a_hand_computed_case():
    """A 3-wide horizontal line from (2, 3) to (8, 3): |y - 3| <= 1.5 for 2 <= x <= 8, and the end discs 4 r^2 <= 9 (r^2 <= 2) add the
    columns 1 and 9.  Then a radius-2 disc about (8, 5), r^2 <= 4, painted later: it wins the four pixels it shares with the line."""
    L_, D = [10, 20, 30], [200, 100, 50]
    calls = [{"type": "line", "p1": [2, 3], "p2": [8, 3], "color": L_, "thickness": 3},
             {"type": "circle", "center": [8, 5], "radius": 2, "color": D}]
    want = ["............",
            "............",
            ".LLLLLLLLL..",
            ".LLLLLLLDL..",
            ".LLLLLLDDD..",
            "......DDDDD.",
            ".......DDD..",
            "........D...",
            "............"]
    got = skel_model.paint(calls, (9, 12))
    colour = {".": [0, 0, 0], "L": L_, "D": D}
    for y, row in enumerate(want):
        for x, ch in enumerate(row):
            assert got[y, x].tolist() == colour[ch], (x, y, ch)
    # painted the other way round the line wins the overlap
    got = skel_model.paint(calls[::-1], (9, 12))
    assert got[3, 8].tolist() == L_ and got[4, 7].tolist() == L_ and got[5, 8].tolist() == D
    # a line of length zero is its end disc; a primitive off the canvas paints nothing; one across the border is clipped
    dot = skel_model.paint([{"type": "line", "p1": [5, 4], "p2": [5, 4], "color": L_, "thickness": 2}], (9, 12))
    assert sorted(map(tuple, np.argwhere(dot.any(axis=2)).tolist())) == [(3, 5), (4, 4), (4, 5), (4, 6), (5, 5)]
    assert not skel_model.paint([{"type": "circle", "center": [40, 40], "radius": 3, "color": D}], (9, 12)).any()
    edge = skel_model.paint([{"type": "circle", "center": [-1, 0], "radius": 2, "color": D}], (9, 12))
    assert sorted(map(tuple, np.argwhere(edge.any(axis=2)).tolist())) == [(0, 0), (0, 1), (1, 0)]


def test_pack_calls_layout():
    rec = skeleton.pack_calls([{"type": "line", "p1": [1, -2], "p2": [3, 4], "color": [5, 6, 7], "thickness": 8},
                               {"type": "circle", "center": [9, 10], "radius": 0, "color": [255, 0, 128]}])
    assert rec.dtype == np.int32 and rec.tolist() == [[0, 1, -2, 3, 4, 8, 5 | 6 << 8 | 7 << 16, 0], [1, 9, 10, 9, 10, 0, 255 | 128 << 16, 0]]


def test_library_exports_the_entry_and_there_is_no_cpu_path():
    lib = L.load()
    assert hasattr(lib, "dm4d_skeleton_draw_u8") and "dm4d_skeleton_draw_u8" in L.SIGNATURES
    t = torch.zeros((1, 8), dtype=torch.int32)
    with pytest.raises(L.Dm4dError, match="HIP device"):
        ops.skeleton_draw(t, t, t, t, t, t, 1, t, t, 1, 8, 8, 8, 8)
    for device in ("cpu", torch.device("cpu")):
        with pytest.raises(L.Dm4dError, match="not a HIP device"):
            skeleton.draw_plans([plan(CASES["scores_only"])], device=device)


def _call(prims, offsets, H=2048, W=2048, h=1024, w=1024, htab=None, vtab=None):
    """dm4d_skeleton_draw_u8 with host memory in every place: only for calls that the host-side validation must refuse (it returns before any
    launch; a call that passed would be given a null output and is refused for that)."""
    lib = L.load()
    hb, hk = bicubic_table(W, w)
    vb, vk = bicubic_table(H, h)
    htab = np.concatenate([hb.reshape(-1), hk.reshape(-1)]).astype(np.int32) if htab is None else htab
    vtab = np.concatenate([vb.reshape(-1), vk.reshape(-1)]).astype(np.int32) if vtab is None else vtab
    prims = np.ascontiguousarray(prims, dtype=np.int32)
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    buf = ctypes.create_string_buffer(prims.nbytes + 16)  # a 16-byte aligned copy
    base = (ctypes.addressof(buf) + 15) & ~15
    ctypes.memmove(base, prims.ctypes.data, prims.nbytes)
    out = np.zeros(16, dtype=np.uint8)
    rc = lib.dm4d_skeleton_draw_u8(None, base, base, offsets.ctypes.data, offsets.ctypes.data, len(offsets) - 1, htab.ctypes.data, htab.ctypes.data,
                                   hk.shape[1], vtab.ctypes.data, vtab.ctypes.data, vk.shape[1], H, W, h, w, out.ctypes.data)
    return rc, lib.dm4d_last_error().decode()


def test_the_entry_validates_its_host_copies_before_launching():
    line = [0, 10, 10, 50, 50, 4, 0x00ff00, 0]
    for rec, what in (([7, 10, 10, 50, 50, 4, 0, 0], "unknown primitive kind"), ([0, 8192, 10, 50, 50, 4, 0, 0], "coordinate"),
                      ([1, 10, -8193, 10, -8193, 4, 0, 0], "coordinate"), ([0, 10, 10, 50, 50, 0, 0, 0], "thickness below 1"),
                      ([1, 10, 10, 10, 10, -1, 0, 0], "negative radius"), ([0, 10, 10, 50, 50, 4, 1 << 24, 0], "colour")):
        rc, msg = _call([line, rec], [0, 2])
        assert rc == -1 and what in msg, (rec, msg)
    rc, msg = _call([line] * 513, [0, 513])
    assert rc == -1 and "DM4D_SKEL_MAX_PRIMS" in msg
    rc, msg = _call([line] * 2, [0, 2, 1])
    assert rc == -1 and "primitive count" in msg
    rc, msg = _call([line], [1, 1])
    assert rc == -1 and "offsets[0]" in msg
    hb, hk = bicubic_table(2048, 1024)
    bad = np.concatenate([hb.reshape(-1), hk.reshape(-1)]).astype(np.int32)
    bad[2 * 1023 + 1] += 1  # the last window now ends one pixel past the canvas
    rc, msg = _call([line], [0, 1], htab=bad)
    assert rc == -1 and "coefficient table" in msg
    bad = np.concatenate([hb.reshape(-1), hk.reshape(-1)]).astype(np.int32)
    bad[2 * 500] = bad[2 * 499] - 1  # window 500 starts (and ends) before window 499, still inside the canvas and no longer than ksize
    assert 0 <= bad[2 * 500] and bad[2 * 500 + 1] <= hk.shape[1]
    rc, msg = _call([line], [0, 1], htab=bad)
    assert rc == -1 and "not ordered" in msg
    rc, msg = _call([line], [0, 1], h=100, w=100)  # a ratio of 20: no tile's footprint fits
    assert rc == -1 and "does not fit in LDS" in msg
    rc, msg = _call([line], [0, 1], H=5000)
    assert rc == -1 and "oversized" in msg
