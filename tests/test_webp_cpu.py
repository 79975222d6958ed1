"""CPU: the definition of the device lossless-WebP encoder (tests/webp_model.py) against an independent decoder.  Every file must load in
Pillow (libwebp) as WEBP / RGB of the right size to exactly the input; the RIFF and chunk sizes and the even padding are read by hand;
the cases' premises (which code forms and paths they take) are checked on the model's pieces; ``code_lengths`` gives complete codes
within the limit for adversarial histograms."""
import functools
import heapq
import io
import struct

import numpy as np
import pytest
from PIL import Image

import webp_cases
import webp_model as M


@functools.lru_cache(maxsize=None)
def all_cases():
    return webp_cases.cases()


def names():
    return sorted(webp_cases.cases())


def unrestricted_depth(hist) -> int:
    """Depth of the deepest leaf of a Huffman tree of the non-zero counts (heapq: an implementation of its own)."""
    heap = [(c, 0) for c in hist if c > 0]
    heapq.heapify(heap)
    while len(heap) > 1:
        (c1, d1), (c2, d2) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (c1 + c2, max(d1, d2) + 1))
    return heap[0][1]


def hists(img):
    return M.histograms(img, *M.tokens(img))


@pytest.mark.parametrize("name", names())
def test_model_file_decodes_to_the_input(name):
    img = all_cases()[name]
    h, w = img.shape[:2]
    f = M.encode(img)
    im = Image.open(io.BytesIO(f))
    im.load()
    assert im.format == "WEBP" and im.mode == "RGB" and im.size == (w, h)
    assert np.array_equal(np.asarray(im), img)
    # the container, by hand
    assert f[:4] == b"RIFF" and f[8:16] == b"WEBPVP8L" and len(f) % 2 == 0
    riff, = struct.unpack("<I", f[4:8])
    payload, = struct.unpack("<I", f[16:20])
    assert riff == len(f) - 8 and riff == 4 + 8 + payload + (payload & 1)
    if payload & 1:
        assert f[-1] == 0
    assert f[20] == 0x2f
    bits = int.from_bytes(f[21:25], "little")
    assert (bits & 0x3fff, (bits >> 14) & 0x3fff, bits >> 28) == (w - 1, h - 1, 0)  # width, height, alpha_is_used + version
    assert len(f) <= M.bound(h, w)


def test_bound_and_stripes_match_the_library():
    from diffuman4d_amd.host import lib as L
    from diffuman4d_amd.host import webp
    lib = L.load()
    assert L.WEBP_STRIPE_PIXELS == M.STRIPE_PIXELS and L.WEBP_MAX_SIDE == M.MAX_SIDE
    for h, w in [(1, 1), (17, 19), (1024, 1024), (16383, 16383), (1, 16383)]:
        assert lib.dm4d_webp_bound(h, w) == M.bound(h, w) > 0
        assert webp.n_stripes(h, w) == M.n_stripes(h, w)
    for h, w in [(0, 1), (1, 0), (16384, 1), (1, 16384), (-1, 5)]:
        assert lib.dm4d_webp_bound(h, w) == 0 and M.bound(h, w) == 0


def test_premises_of_the_cases():
    cs = all_cases()
    # one pixel: every code has one symbol, so after the tables there is not one bit (the only image with a stripe of 0 bits)
    one = cs["noise_1x1"]
    tables = sum(sum(M.code_table(h)[1]) for h in hists(one))
    assert len(M.payload(one)) == (43 + tables + 7) // 8 and all(max(M.code_table(h)[2]) == 0 for h in hists(one))
    # one colour: three tokens; red, blue and alpha cost nothing; the green code holds the literal and two length prefixes, the
    # distance code both plane codes, so the three tokens cost 2 + (2 + 4 + 1) + (1 + 10 + 1) bits or so -- not zero
    pos, kind, length = M.tokens(cs["constant"])
    assert kind.tolist() == [M.LITERAL, M.LEFT, M.UP] and length.tolist() == [1, 63, 4032]
    g, r, b, a, d = hists(cs["constant"])
    assert all(max(M.code_table(h)[2]) == 0 for h in (r, b, a)) and sorted(v for v in M.code_table(g)[2] if v) == [1, 2, 2]
    tables = sum(sum(M.code_table(h)[1]) for h in (g, r, b, a, d))
    extra = M.prefix(63)[1] + M.prefix(4032)[1]
    assert len(M.payload(cs["constant"])) == (43 + tables + (1 + 2 + 2) + extra + 2 + 7) // 8
    # two colours: red, blue and green literals go through simple codes of two symbols
    g, r, b, a, d = hists(cs["two_colours"])
    assert sum(1 for c in r if c) == 2 and sum(1 for c in b if c) == 2
    assert M.code_table(r)[0][:2] == [1, 1] and M.code_table(b)[0][:2] == [1, 1] and M.code_table(a)[0] == [1, 0, 1, 255]
    # width 1: no pixel is of kind L, the pixel above is the pixel before
    assert M.LEFT not in M.tokens(cs["column"])[1] and M.UP in M.tokens(cs["column"])[1]
    # noise: literals only; the distance code is the empty one; normal codes over most of 256 symbols
    pos, kind, length = M.tokens(cs["noise_17x33"])
    assert (kind == M.LITERAL).all() and pos.tolist() == list(range(17 * 33))
    g, r, b, a, d = hists(cs["noise_17x33"])
    assert sum(1 for c in g if c) > 200 and M.code_table(g)[0][0] == 0 and M.code_table(d)[0] == [1, 0, 0, 0]
    # a run of 6400 pixels from 7600 on: cut at the stripe boundary 8192, then after 4096
    pos, kind, length = M.tokens(cs["long_run"])
    at = np.flatnonzero(pos == 7600)[0]
    assert kind[at:at + 3].tolist() == [M.UP] * 3 and pos[at:at + 4].tolist() == [7600, 8192, 8192 + 4096, 14000]
    assert length[at:at + 3].tolist() == [592, 4096, 6400 - 592 - 4096]
    assert M.stripe_pixels(150, 100) == 8192 and M.n_stripes(150, 100) == 2
    assert M.n_stripes(*cs["striped"].shape[:2]) == 3
    # the Fibonacci-shaped green histogram: an unrestricted Huffman code is deeper than 15 bits, the model's is not
    g = hists(cs["fibonacci"])[0]
    assert (M.tokens(cs["fibonacci"])[1] == M.LITERAL).all()
    assert sum(1 for c in g if c) >= 17 and unrestricted_depth(g) > 15 and max(M.code_lengths(g, 15)) <= 15
    assert cs["widest"].shape == (1, 16383, 3) and M.n_stripes(1, 16383) == 2
    # the drawn map: mostly black, with anti-aliased strokes
    sk = cs["skeleton_map"]
    assert sk.shape == (64, 48, 3) and (sk.reshape(-1, 3).max(axis=1) == 0).mean() > 0.5 and len(np.unique(sk.reshape(-1, 3), axis=0)) > 50


def test_deep_literals_keep_reaching_the_third_window_word():
    """A condition on the input, not on the device: the emitter ORs a token of nb bits into its window of 32-bit words at bit `pos`,
    counted from the byte in which its round starts (a round is 2048 pixels within a stripe), and a token with (pos & 31) + nb > 64
    spills into a third word.  "deep_literals" is the case that has such tokens: 10 of them, by the model's own code lengths and
    token order, and tokens of 45 bits, the format's maximum."""
    img = all_cases()["deep_literals"]
    pos, kind, length = M.tokens(img)
    assert img.shape == (4, 2583, 3) and M.n_stripes(4, 2583) == 2 and int((kind == M.LITERAL).sum()) == 10329
    tables = [M.code_table(h) for h in M.histograms(img, pos, kind, length)]
    lens = [np.array(t[2], dtype=np.int64) for t in tables]
    px = img.reshape(-1, 3).astype(np.int64)[pos]
    lit = lens[0][px[:, 1]] + lens[1][px[:, 0]] + lens[2][px[:, 2]] + lens[3][255]
    pre = np.array([M.prefix(int(v)) for v in length], dtype=np.int64)
    ref = lens[0][256 + pre[:, 0]] + pre[:, 1] + lens[4][np.where(kind == M.UP, 0, 1)]
    nb = np.where(kind == M.LITERAL, lit, ref)
    start = 43 + sum(sum(t[1]) for t in tables) + np.cumsum(nb) - nb  # the first bit of every token in the payload
    rnd = pos // M.STRIPE_PIXELS * M.STRIPE_PIXELS + pos % M.STRIPE_PIXELS // 2048 * 2048
    first = np.flatnonzero(np.append(True, rnd[1:] != rnd[:-1]))  # a round's first token
    origin = (start[first] // 8 * 8)[np.cumsum(np.append(True, rnd[1:] != rnd[:-1])) - 1]
    sh = (start - origin) % 32
    assert int(nb.max()) == 45
    assert int((sh + nb > 64).sum()) >= 5


def test_prefix_of_lengths_and_plane_codes():
    assert [M.prefix(v) for v in (1, 2, 3, 4)] == [(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0)]
    assert M.prefix(5) == (4, 1, 0) and M.prefix(6) == (4, 1, 1) and M.prefix(7) == (5, 1, 0) and M.prefix(9) == (6, 2, 0)
    assert M.prefix(4096) == (23, 10, 1023) and M.prefix(3073) == (23, 10, 0) and M.prefix(3072) == (22, 10, 1023)
    # every length is its prefix's base plus the extra value, and the bases are increasing
    seen = {}
    for v in range(1, 4097):
        s, eb, ev = M.prefix(v)
        assert 0 <= s < 24 and 0 <= ev < (1 << eb)
        seen.setdefault(s, v - ev)
        assert seen[s] == v - ev
    assert sorted(seen.values()) == [seen[s] for s in sorted(seen)] and len(seen) == 24


ADVERSARIAL = {
    "fibonacci_30": [1, 1] + [0] * 3 + [2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4181, 6765, 10946, 17711, 28657, 46368,
                                      75025, 121393, 196418, 317811, 514229, 832040],
    "powers_of_two": [1 << k for k in range(24)],
    "one_huge": [1] * 279 + [1 << 30],
    "all_equal": [7] * 280,
    "all_equal_odd": [3] * 19,
    "two": [0, 5, 0, 0, 9],
    "two_equal": [4, 4],
    "three": [1, 1, 1],
    "steps": [1] * 100 + [1000] * 100 + [1000000] * 80,
    "tail_of_ones": [1 << 20] + [1] * 255,
}


@pytest.mark.parametrize("name", sorted(ADVERSARIAL))
@pytest.mark.parametrize("limit", [15, 7])
def test_code_lengths_within_the_limit_and_complete(name, limit):
    hist = ADVERSARIAL[name][:19] if limit == 7 else ADVERSARIAL[name]   # the code-length code has 19 symbols
    lens = M.code_lengths(hist, limit)
    assert len(lens) == len(hist) and all((c > 0) == (v > 0) for c, v in zip(hist, lens))
    assert max(lens) <= limit
    if sum(1 for c in hist if c) >= 2:
        assert sum(2 ** (limit - v) for v in lens if v) == 2 ** limit  # Kraft with equality: a complete code


def test_code_lengths_random_histograms():
    rng = np.random.default_rng(3)
    for limit, n in ((15, 280), (15, 256), (15, 40), (7, 19)):
        for _ in range(25):
            hist = (rng.integers(1, 1 << int(rng.integers(1, 28)), n) * (rng.random(n) < rng.random())).tolist()
            hist[0] += 1
            hist[n - 1] += 1
            lens = M.code_lengths(hist, limit)
            assert all((c > 0) == (v > 0) for c, v in zip(hist, lens)) and max(lens) <= limit
            assert sum(2 ** (limit - v) for v in lens if v) == 2 ** limit
