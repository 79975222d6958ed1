"""The definition of the keypoint stage's arithmetic (diffuman4d_amd/csrc/pose.hip, host/pose.py), in numpy + scipy, written from
DESIGN.md "Keypoint prediction": the box -> centre / scale / UDP matrix, the integer warp with its composite, the normalisation through
torch CPU, and the UDP/DARK decode parametrised by dtype (float64 is the yardstick, float32 restates the reference's own precision).
Slow and plain on purpose: loops over pixels where that is the clearest form."""
import numpy as np
import torch
from scipy.ndimage import correlate1d

MEAN = (123.5, 116.5, 103.5)
STD = (58.5, 57.0, 57.5)
PADDING = 1.25


# -- box -> centre, scale, matrix ----------------------------------------------------------------------------------------------------
def center_scale(box, shape, padding=PADDING):
    """[x1, y1, x2, y2] and the network input (H, W) -> centre (2,), scale (2,) in float64: the padded box grown to the input's aspect."""
    x1, y1, x2, y2 = (np.float64(v) for v in box)
    H, W = shape
    center = np.array([x1 + x2, y1 + y2]) * 0.5
    bw, bh = (x2 - x1) * padding, (y2 - y1) * padding
    aspect = W / H
    scale = np.array([bw, bw / aspect]) if bw > bh * aspect else np.array([bh * aspect, bh])
    return center, scale


def udp_matrix(center, scale, shape):
    """The 2 x 3 float32 matrix image -> network input without rotation.  Per axis the box edge centre - scale / 2 goes to 0 and the edge
    centre + scale / 2 to the last pixel (unbiased data processing: edges map to pixel centres): gain k = last / scale, offset
    k (scale / 2 - centre), both formed in float64 and rounded to float32 when stored."""
    H, W = shape
    m = np.zeros((2, 3), dtype=np.float32)
    for axis, last in enumerate((W - 1, H - 1)):
        k = last / scale[axis]
        m[axis, axis] = k
        m[axis, 2] = k * (scale[axis] / 2 - center[axis])
    return m


def warp_tables(m, shape):
    """The matrix -> (adelta [W], bdelta [W], X0 [H], Y0 [H]) int64: its fp64 inverse (adjugate / determinant) in 10-bit fixed point."""
    H, W = shape
    m = m.astype(np.float64)
    det = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
    d = 1.0 / det if det != 0 else 0.0
    a00, a01, a10, a11 = m[1, 1] * d, m[0, 1] * -d, m[1, 0] * -d, m[0, 0] * d
    a02 = -a00 * m[0, 2] - a01 * m[1, 2]
    a12 = -a10 * m[0, 2] - a11 * m[1, 2]
    xs, ys = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    adelta = np.rint(a00 * xs * 1024).astype(np.int64)
    bdelta = np.rint(a10 * xs * 1024).astype(np.int64)
    X0 = np.rint((a01 * ys + a02) * 1024).astype(np.int64) + 16
    Y0 = np.rint((a11 * ys + a12) * 1024).astype(np.int64) + 16
    return adelta, bdelta, X0, Y0


def weight_table():
    """[32 (fy), 32 (fx), 4] int: the bilinear weights of the taps (0,0), (1,0), (0,1), (1,1) at 1/32-pixel fractions, scale 32768."""
    f = np.arange(32)
    wx = np.stack([32 - f, f], axis=-1)  # [32, 2] in 1/32
    tab = np.zeros((32, 32, 4), dtype=np.int64)
    for fy in range(32):
        for fx in range(32):
            tab[fy, fx] = [32 * wx[fx, 0] * wx[fy, 0], 32 * wx[fx, 1] * wx[fy, 0], 32 * wx[fx, 0] * wx[fy, 1], 32 * wx[fx, 1] * wx[fy, 1]]
    return tab


def composite(p, m):
    """Image.composite(image, black, mask) per byte for an L mask."""
    t = p.astype(np.int64) * m.astype(np.int64) + 128
    return ((t >> 8) + t) >> 8


def warp(image, mask, tables, shape):
    """image uint8 [h, w, 3], mask uint8 [h, w] or None -> int64 [H, W, 3] in 0..255: the integer warp of the composited image."""
    H, W = shape
    h, w = image.shape[:2]
    src = image.astype(np.int64)
    if mask is not None:
        src = composite(src, mask[..., None])
    adelta, bdelta, X0, Y0 = tables
    tab = weight_table()
    out = np.zeros((H, W, 3), dtype=np.int64)
    for y in range(H):
        for x in range(W):
            X, Y = (X0[y] + adelta[x]) >> 5, (Y0[y] + bdelta[x]) >> 5
            sx, sy = X >> 5, Y >> 5
            wts = tab[Y & 31, X & 31]
            acc = np.zeros(3, dtype=np.int64)
            for k, (dx, dy) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
                px, py = sx + dx, sy + dy
                if 0 <= px < w and 0 <= py < h:
                    acc += wts[k] * src[py, px]
            out[y, x] = (acc + (1 << 14)) >> 15
    return out


def normalise(v):
    """int [H, W, 3] -> float32 [3, H, W] (planes R, G, B) through torch CPU: (v.float() - mean) / std."""
    t = torch.from_numpy(np.ascontiguousarray(v.transpose(2, 0, 1))).float()
    return ((t - torch.tensor(MEAN).view(-1, 1, 1)) / torch.tensor(STD).view(-1, 1, 1)).numpy()


def pose_input(image, mask, box, shape, padding=PADDING):
    """One row of the network's input -> (float32 [3, H, W], centre, scale)."""
    h, w = image.shape[:2]
    box = [0, 0, w, h] if box is None else box
    center, scale = center_scale(box, shape, padding)
    tables = warp_tables(udp_matrix(center, scale, shape), shape)
    return normalise(warp(image, mask, tables, shape)), center, scale


def mask_box(mask):
    """[x1, y1, x2, y2] of the pixels >= 128, the whole image for a mask without one."""
    ys, xs = np.nonzero(mask >= 128)
    if len(ys) == 0:
        return [0, 0, mask.shape[1], mask.shape[0]]
    return [int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1]


# -- decode ----------------------------------------------------------------------------------------------------------------------------
def gaussian_taps(dtype, ksize=11):
    sigma = 0.3 * ((ksize - 1) * 0.5 - 1) + 0.8
    x = np.arange(ksize, dtype=np.float64) - (ksize - 1) // 2
    g = np.exp(-(x * x) / (2 * sigma * sigma))
    return (g / g.sum()).astype(dtype)


def udp_decode(heatmaps, dtype=np.float64, details=False):
    """heatmaps float32 [K, Hh, Wh] -> (locations [K, 2] in heatmap pixels, scores float32 [K]); with details also the float64 condition
    number of each map's Hessian + eps I (1 for a map that is not refined).  dtype float64: every step in float64, nothing rounded at
    the end.  dtype float32: the blur, the rescale, clip, log and the five differences in float32, the 2 x 2 solve in float64, the
    location rounded to float32 once."""
    K, Hh, Wh = heatmaps.shape
    taps = gaussian_taps(dtype)
    eps = np.float64(np.finfo(np.float32).eps)
    locs = np.zeros((K, 2), dtype=dtype)
    scores = np.zeros(K, dtype=np.float32)
    conds = np.ones(K, dtype=np.float64)
    for k in range(K):
        hm = heatmaps[k]
        flat = int(np.argmax(hm))
        ay, ax = divmod(flat, Wh)
        scores[k] = hm[ay, ax]
        if not scores[k] > 0:
            locs[k] = -1
            continue
        blurred = correlate1d(correlate1d(hm.astype(dtype), taps, axis=1, mode="constant", cval=0.0), taps, axis=0, mode="constant", cval=0.0)
        blurred = blurred * (dtype(scores[k]) / blurred.max())
        logs = np.log(np.clip(blurred, dtype(1e-3), dtype(50.0)))
        pad = np.pad(logs, 1, mode="edge")

        def lg(ox, oy):
            return pad[ay + 1 + oy, ax + 1 + ox]
        # centre c, neighbours l / r (x -+ 1), u / d (y -+ 1), ul (x - 1, y - 1), dr (x + 1, y + 1); every operation rounded in dtype, in
        # the order DESIGN.md states
        c, l, r, u, d, ul, dr = lg(0, 0), lg(-1, 0), lg(1, 0), lg(0, -1), lg(0, 1), lg(-1, -1), lg(1, 1)
        half, two = dtype(0.5), dtype(2.0)
        gx, gy = (r - l) * half, (d - u) * half
        hxx, hyy = (r - c * two) + l, (d - c * two) + u
        cross = dr
        for term in (-r, -d, c, c, -l, -u, ul):  # added to dr one by one, in this order
            cross = cross + term
        hxy = cross * half
        hess = np.array([[hxx, hxy], [hxy, hyy]], dtype=np.float64) + eps * np.eye(2)
        conds[k] = np.linalg.cond(hess)
        step = np.linalg.inv(hess) @ np.array([gx, gy], dtype=np.float64)
        locs[k] = (np.array([ax, ay], dtype=np.float64) - step).astype(dtype)
    return (locs, scores, conds) if details else (locs, scores)


def to_image(locs, heatmap_size, input_size, center, scale):
    """Heatmap pixels -> image pixels in float64: kp / [Wh - 1, Hh - 1] * input_size, then (kp / input_size) * scale + centre - scale / 2."""
    Wh, Hh = heatmap_size
    kp = (locs.astype(np.float64) if locs.dtype != np.float32 else locs) / [Wh - 1, Hh - 1] * input_size
    return (kp / input_size) * scale + center - 0.5 * scale
