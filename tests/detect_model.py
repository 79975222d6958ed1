"""The definition of the person-box stage's arithmetic (diffuman4d_amd/csrc/detect.hip, host/detect.py), in numpy, written from
DESIGN.md "Person boxes": the keep-ratio size, the per-axis tables, the composite, the integer bilinear resize, pad and normalisation
through torch CPU; and the selection: threshold, rescale, drop, order, cap, greedy NMS in float32.  Plain on purpose."""
import numpy as np
import torch

MEAN = (103.53, 116.28, 123.675)
STD = (57.375, 57.12, 58.395)
PAD_VALUE = 114
ONE = 2048


# -- size and tables -------------------------------------------------------------------------------------------------------------------
def rescaled_size(h, w, shape):
    """(nw, nh) of an h x w image in the canvas shape = (H, W): mmcv's rescale_size with scale = (W, H)."""
    H, W = shape
    sf = min(max(H, W) / max(h, w), min(H, W) / min(h, w))
    return int(w * sf + 0.5), int(h * sf + 0.5)


def fits(h, w, shape):
    nw, nh = rescaled_size(h, w, shape)
    return 1 <= nw <= shape[1] and 1 <= nh <= shape[0]


def positions(src, dst):
    """The sampling positions of one axis as float64 values of float32: fp32((d + 0.5) * (src / dst) - 0.5)."""
    return np.array([np.float64(np.float32((d + 0.5) * (src / dst) - 0.5)) for d in range(dst)])


def axis(src, dst):
    """-> (s [dst], c0 [dst], c1 [dst]) int: the first tap and the weights of the taps s and s + 1."""
    s, c0, c1 = [], [], []
    for f in positions(src, dst):
        k = int(np.floor(f))
        a = f - k
        if k < 0:
            k, a = 0, 0.0
        if k >= src - 1:
            k, a = src - 1, 0.0
        s.append(k), c1.append(int(min(max(np.rint(a * ONE), -32768), 32767))), c0.append(int(min(max(np.rint((1.0 - a) * ONE), -32768), 32767)))
    return np.array(s), np.array(c0), np.array(c1)


def inv_scale(h, w, shape):
    nw, nh = rescaled_size(h, w, shape)
    return np.float32(1.0 / (nw / w)), np.float32(1.0 / (nh / h))


# -- the input -------------------------------------------------------------------------------------------------------------------------
def composite(p, m):
    """Image.composite(image, black, mask) per byte for an L mask."""
    t = p.astype(np.int64) * m.astype(np.int64) + 128
    return ((t >> 8) + t) >> 8


def resize(image, nw, nh):
    """int [h, w, 3] -> int64 [nh, nw, 3]: horizontal pass S = p[s] c0 + p[s + 1] c1 (second tap clamped), then
    (((b0 (S0 >> 4)) >> 16) + ((b1 (S1 >> 4)) >> 16) + 2) >> 2 over the rows s and s + 1 (clamped)."""
    h, w = image.shape[:2]
    src = image.astype(np.int64)
    xs, a0, a1 = axis(w, nw)
    ys, b0, b1 = axis(h, nh)
    S = src[:, xs] * a0[None, :, None] + src[:, np.minimum(xs + 1, w - 1)] * a1[None, :, None]  # [h, nw, 3]
    S0, S1 = S[ys] >> 4, S[np.minimum(ys + 1, h - 1)] >> 4
    return (((b0[:, None, None] * S0) >> 16) + ((b1[:, None, None] * S1) >> 16) + 2) >> 2


def canvas_bytes(image, mask, shape, pad_value=PAD_VALUE):
    """uint8 [h, w, 3] image, uint8 [h, w] mask or None -> int64 [H, W, 3]: the resized composite in the top-left corner, pad elsewhere."""
    H, W = shape
    h, w = image.shape[:2]
    nw, nh = rescaled_size(h, w, shape)
    assert 1 <= nw <= W and 1 <= nh <= H
    src = image.astype(np.int64)
    if mask is not None:
        src = composite(src, mask[..., None])
    out = np.full((H, W, 3), pad_value, dtype=np.int64)
    out[:nh, :nw] = resize(src, nw, nh)
    return out


def detector_input(image, mask, shape, mean=MEAN, std=STD, pad_value=PAD_VALUE, channel_order="rgb"):
    """-> float32 [3, H, W] through torch CPU: plane c = (v[c] - mean[c]) / std[c], v[c] the RGB channel c ("bgr": 2 - c)."""
    v = canvas_bytes(image, mask, shape, pad_value)
    if channel_order == "bgr":
        v = v[..., ::-1]
    t = torch.from_numpy(np.ascontiguousarray(v.transpose(2, 0, 1))).float()
    return ((t - torch.tensor(mean, dtype=torch.float32).view(-1, 1, 1)) / torch.tensor(std, dtype=torch.float32).view(-1, 1, 1)).numpy()


# -- the selection ---------------------------------------------------------------------------------------------------------------------
def nms(dets, thr):
    """dets float32 [k, 5] (x1, y1, x2, y2, score) in the order of visiting -> the kept row numbers.  Greedy, float32, every operation
    rounded on its own; a later box survives iff ovr <= thr."""
    f = np.float32
    dets, thr = np.asarray(dets, dtype=np.float32).reshape(-1, 5), f(thr)
    alive = [True] * len(dets)
    area = [f(f(f(d[2] - d[0]) + f(1)) * f(f(d[3] - d[1]) + f(1))) for d in dets]
    keep = []
    with np.errstate(all="ignore"):
        for i, di in enumerate(dets):
            if not alive[i]:
                continue
            keep.append(i)
            for j in range(i + 1, len(dets)):
                if not alive[j]:
                    continue
                dj = dets[j]
                w = max(f(0), f(f(min(di[2], dj[2]) - max(di[0], dj[0])) + f(1)))
                h = max(f(0), f(f(min(di[3], dj[3]) - max(di[1], dj[1])) + f(1)))
                inter = f(w * h)
                ovr = f(inter / f(f(area[i] + area[j]) - inter))
                if not ovr <= thr:
                    alive[j] = False
    return keep


def select(boxes, scores, inv, cat=0, score_thr=0.3, nms_thr=0.3, max_per_img=100):
    """boxes float32 [A, 4], scores float32 [A, C], inv = (inv_w, inv_h) float32 -> (counts [kept, dropped, above], float32
    [max_per_img, 5], int32 [max_per_img]) as include/dm4d.h states them."""
    f = np.float32
    boxes, scores = np.asarray(boxes, dtype=np.float32), np.asarray(scores, dtype=np.float32)
    s = scores[:, cat]
    with np.errstate(all="ignore"):
        above = np.nonzero(s > f(score_thr))[0]                                 # NaN > thr is False
        img = (boxes[above] * np.array([inv[0], inv[1], inv[0], inv[1]], dtype=np.float32)).astype(np.float32)
    ok = np.isfinite(img).all(axis=1) & (img[:, 2] > img[:, 0]) & (img[:, 3] > img[:, 1])
    cand, img = above[ok], img[ok]
    order = sorted(range(len(cand)), key=lambda k: (-np.float64(s[cand[k]]), cand[k]))[:max_per_img]  # -0.0 == 0.0 here, as on the device
    dets = np.concatenate([img[order], s[cand[order]][:, None]], axis=1).astype(np.float32) if order else np.zeros((0, 5), np.float32)
    keep = nms(dets, nms_thr)
    out, idx = np.zeros((max_per_img, 5), dtype=np.float32), np.full(max_per_img, -1, dtype=np.int32)
    out[:len(keep)] = dets[keep]
    idx[:len(keep)] = cand[order][keep] if keep else []
    return [len(keep), int(len(above) - len(cand)), int(len(above))], out, idx
