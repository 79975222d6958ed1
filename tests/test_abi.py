"""CPU: the C-ABI shared library loads (no GPU needed) and exports every symbol include/dm4d.h declares;
the ctypes prototype table in diffuman4d_amd/host/lib.py covers exactly that set with matching arity."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "dm4d.h").read_text()


def header_functions():
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(?:int|size_t|const char\s*\*)\s+(dm4d_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S):
        args = m.group(2).strip()
        n = 0 if args in ("", "void") else len([a for a in args.split(",") if a.strip()])
        out[m.group(1)] = n
    return out


def test_header_declares_the_expected_surface():
    fns = header_functions()
    for name in ("dm4d_gemm_bf16", "dm4d_conv3x3_nhwc_bf16", "dm4d_attention_bf16", "dm4d_groupnorm_nhwc_bf16",
                 "dm4d_layernorm_bf16", "dm4d_pack_model_input_bf16", "dm4d_cfg_ddim_step_bf16"):
        assert name in fns


def test_library_builds_loads_and_exports_every_symbol():
    from diffuman4d_amd import build
    lib_path = build.build(force=False, verbose=False)
    lib = ctypes.CDLL(str(lib_path))
    for name in header_functions():
        assert hasattr(lib, name), f"{name} declared in dm4d.h but not exported by {lib_path.name}"
    lib.dm4d_version.restype = ctypes.c_int
    assert lib.dm4d_version() >= 100


def test_ctypes_table_matches_header():
    from diffuman4d_amd.host import lib as L
    fns = header_functions()
    assert set(L.SIGNATURES) == set(fns)
    for name, (_, argtypes) in L.SIGNATURES.items():
        assert len(argtypes) == fns[name], f"{name}: header has {fns[name]} args, ctypes table {len(argtypes)}"
    L.load()


def test_ops_refuse_cpu_tensors():
    """There is no CPU fallback: a host tensor is an error, never a silent slow path."""
    import torch
    from diffuman4d_amd.host import lib as L, ops
    a = torch.zeros(32, 32, dtype=torch.bfloat16)
    with pytest.raises(L.Dm4dError, match="HIP device"):
        ops.gemm(a, a)
    with pytest.raises(L.Dm4dError, match="HIP device"):
        ops.layernorm(a, a[0], a[0])


def test_conv_split_decision_depends_on_the_image_not_on_the_batch():
    """dm4d_conv3x3_ws_bytes (host-only query): the split over the kernel rows applies to small images with a deep K
    (the 9x5 level) and to stride-1 'same' convolutions only, and whether it applies never depends on B -- a
    frame-sharded rank convolves fewer images per launch and must sum in the same order as the unsharded run."""
    from diffuman4d_amd.host import lib as L
    lib = L.load()

    def ws(B, H, W, Cin, Cout, stride=1, pad=1, up=0, Ho=None, Wo=None):
        Ho, Wo = (H if Ho is None else Ho), (W if Wo is None else Wo)
        return lib.dm4d_conv3x3_ws_bytes(B, H, W, Cin, Ho, Wo, Cout, stride, pad, up)

    for B in (1, 2, 3, 32, 48):
        assert ws(B, 9, 5, 1280, 1280) == 3 * B * 45 * 1280 * 4      # three fp32 partial planes
        assert ws(B, 9, 5, 2560, 1280) == 3 * B * 45 * 1280 * 4
        assert ws(B, 8, 8, 512, 128) == 3 * B * 64 * 128 * 4
        assert ws(B, 18, 10, 1280, 1280) == 0                        # 180 pixels: enough rows, never split
        assert ws(B, 9, 5, 256, 1280) == 0                           # shallow K
        assert ws(B, 9, 5, 1280, 1280, stride=2, Ho=5, Wo=3) == 0    # stride 2 is not a strip convolution
        assert ws(B, 9, 5, 1280, 1280, up=1, Ho=18, Wo=10) == 0      # neither is the fused up-sampling
        assert ws(B, 9, 5, 1280, 1284) == 0                          # N not a multiple of 8: no vector epilogue


def test_a_stale_library_is_not_blessed(monkeypatch, tmp_path):
    """`needs_build()` compares the content hash recorded when libdm4d.so was linked with the hash of the sources in the tree (file times do
    not survive the copy to a GPU box): one changed byte in a kernel source, a header or a compile flag makes the library stale, and
    `__graft_entry__.build()` asserts on exactly this predicate after building."""
    from diffuman4d_amd import build
    build.build(force=False, verbose=False)
    assert not build.needs_build()
    h0 = build.source_hash()
    # a different recorded hash (= the library was linked from other sources)
    stamp = tmp_path / "stamp"
    stamp.write_text("0" * 64)
    monkeypatch.setattr(build, "STAMP", stamp)
    assert build.needs_build()
    stamp.write_text(h0)
    assert not build.needs_build()
    # one more byte in a source: the tree's hash moves, the recorded one does not
    fake = tmp_path / "csrc"
    fake.mkdir()
    for f in list(build.CSRC.glob("*.hip")) + list(build.CSRC.glob("*.h")):
        (fake / f.name).write_bytes(f.read_bytes())
    (fake / build.SOURCES[0]).write_bytes((fake / build.SOURCES[0]).read_bytes() + b"\n")
    monkeypatch.setattr(build, "CSRC", fake)
    assert build.source_hash() != h0 and build.needs_build()
    # a missing stamp is stale too
    monkeypatch.setattr(build, "CSRC", build.ROOT / "csrc")
    monkeypatch.setattr(build, "STAMP", tmp_path / "absent")
    assert build.needs_build()


# the constants of include/dm4d.h that diffuman4d_amd/host/lib.py mirrors (without the DM4D_ prefix): they size descriptor rows and
# workspaces that the library indexes, so a mirror that is deleted or renamed must fail here, not on a device
MIRRORED = ("EPI_GEGLU", "EPI_SILU", "EPI_F32OUT", "EPI_F32SIDE", "EPI_SPLITOUT", "LOG2E", "CAPTURE_FIELDS", "EVAL_FIELDS", "EVAL_OUT",
            "EVAL_IMAGE_F32", "EVAL_MASK_F32", "EVAL_CROP_MASKS", "EVAL_BG_SHIFT", "LPIPS_TAPS", "LPIPS_IN_COLS", "VHULL_BLOCK",
            "VHULL_MAX_CHUNK", "TRIANG_MAX_VIEWS", "SKEL_FIELDS", "SKEL_LINE", "SKEL_CIRCLE", "SKEL_MAX_PRIMS", "SKEL_COORD_MIN",
            "SKEL_COORD_MAX", "RESTORE_FIELDS", "JPEG_FIELDS", "JPEG_MCU_UNSTUFFED", "JPEG_MCU_BOUND", "JPEG_CHUNK")


def _constant(text: str):
    """Value of a #define's replacement text: an integer literal (decimal or hex, u / l / ll suffixes), unary minus, `<<`, parentheses;
    or a plain decimal float.  Anything else is a ValueError."""
    integer = r"(?:0[xX][0-9a-fA-F]+|\d+)(?:[uU](?:ll|LL|l|L)?|(?:ll|LL|l|L)[uU]?)?"
    real = r"\d+\.\d+(?:[eE][-+]?\d+)?"
    tokens = re.findall(real + "|" + integer + r"|<<|[-()]|\S", text)
    pos = 0

    def peek():
        return tokens[pos] if pos < len(tokens) else None

    def take():
        nonlocal pos
        pos += 1
        return tokens[pos - 1]

    def unary():
        tok = take() if peek() is not None else ""
        if tok == "-":
            return -unary()
        if tok == "(":
            v = shift()
            if peek() != ")":
                raise ValueError(text)
            take()
            return v
        if re.fullmatch(real, tok):
            return float(tok)
        if re.fullmatch(integer, tok):
            return int(tok.rstrip("uUlL"), 0)
        raise ValueError(text)

    def shift():
        v = unary()
        while peek() == "<<":
            take()
            n = unary()
            if not (isinstance(v, int) and isinstance(n, int) and 0 <= n < 64):
                raise ValueError(text)
            v <<= n
        return v

    v = shift()
    if pos != len(tokens):
        raise ValueError(text)
    return v


def header_constants():
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    return {m.group(1): m.group(2).strip() for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+DM4D_(\w+)[ \t]+(\S[^\n]*)$", text, flags=re.M)}


def test_constant_parser():
    assert [_constant(t) for t in ("16", "4u", "(1ll << 26)", "(-8192)", "0x10", "-(2 << 3)", "1ULL<<4", "1.4426950408889634")] == [
        16, 4, 1 << 26, -8192, 16, -16, 16, 1.4426950408889634]
    for bad in ("", "1 +", "(1", "A", "1 2", "1.5 << 2", "sizeof(int)"):
        with pytest.raises(ValueError):
            _constant(bad)


def test_mirrored_constants_match_header():
    """Every DM4D_* constant that host/lib.py holds has the header's value, and host/lib.py holds at least the MIRRORED ones."""
    from diffuman4d_amd.host import lib as L
    consts = header_constants()
    for name in MIRRORED:
        assert name in consts, f"DM4D_{name} is not defined in include/dm4d.h"
        assert hasattr(L, name), f"diffuman4d_amd/host/lib.py does not mirror DM4D_{name}"
    checked = 0
    for name, text in consts.items():
        if hasattr(L, name):
            want, got = _constant(text), getattr(L, name)
            assert type(got) is type(want) and got == want, f"host/lib.py {name} = {got!r}, include/dm4d.h DM4D_{name} = {text}"
            checked += 1
    assert checked >= len(MIRRORED)
