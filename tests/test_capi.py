"""The C-ABI library loads on a CPU-only host and exports exactly what
include/recblr_hip.h declares (no compute call is made here), and the ctypes
prototypes derived from the headers are what the headers say."""
import ctypes
import os
import re

import pytest

from datamining_recblr_amd import _lib

_i64, _p, _int = ctypes.c_int64, ctypes.c_void_p, ctypes.c_int
_f32, _f64, _u64 = ctypes.c_float, ctypes.c_double, ctypes.c_uint64


def header_functions():
    text = open(_lib.HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.findall(r"\b(rb_[a-z0-9_]+)\s*\(", text)


def test_header_declares_expected_entry_points():
    names = header_functions()
    assert len(names) == len(set(names))
    assert set(names) == set(_lib.SIGNATURES), set(names) ^ set(_lib.SIGNATURES)
    assert list(_lib.SIGNATURES) == names          # header order
    assert (len(_lib.SIGNATURES), len(_lib.EXP_SIGNATURES), len(_lib.PROBE_SIGNATURES)) == (63, 4, 3)
    for must in ("rb_scan_fwd", "rb_scan_bwd", "rb_conv_silu_fwd", "rb_conv_silu_bwd",
                 "rb_gate_scan_fwd", "rb_gate_scan_bwd", "rb_version", "rb_last_error_string"):
        assert must in names


def test_library_loads_and_exports_every_symbol():
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in header_functions():
        assert hasattr(raw, name), name
    assert lib.rb_version() == _lib.ABI_VERSION
    assert lib.rb_num_kernels() > 0


def test_tile_constant_matches_header():
    text = open(_lib.HEADER_PATH).read()
    assert re.search(r"#define RB_TILE (\d+)", text).group(1) == str(_lib.RB_TILE)
    assert re.search(r"#define RB_EINVAL \((-?\d+)\)", text).group(1) == str(_lib.RB_EINVAL)
    # Python code sizes buffers and reads statuses with these
    assert _lib.RB_TILE == 16 and _lib.RB_EINVAL == -1
    assert re.search(r"#define RB_ABI_VERSION (\d+)", text).group(1) == str(_lib.ABI_VERSION)


# prototypes written out by hand, one of each kind of argument and return
PINNED = {
    "rb_scan_fwd": (_int, [_p, _p, _p, _i64, _i64, _i64, _p]),
    "rb_add_ln_fwd": (_int, [_p, _p, _i64, _p, _u64, _f32, _p, _p, _p, _f32, _p, _p, _p, _p, _i64,
                             _i64, _p]),
    "rb_adam_step": (_int, [_p, _i64, _f64, _f64, _f64, _f64, _f64, _f64, _f64, _p]),
    "rb_pad_prefix_bwd": (_int, [_p, _p, _p, _p, _p, _i64, _i64, _i64, _p, _p, _p, _p, _p, _p,
                                 _int, _p]),
    "rb_gemm_nt_h_mode": (_int, [_int]),
    "rb_row_num_parts": (_i64, [_i64, _i64]),
    "rb_last_error_string": (ctypes.c_char_p, []),
    "rb_item_topk": (_int, [_p, _p, _i64, _i64, _i64, _i64, _i64, _p, _i64, _p, _p, _p, _i64, _p]),
    "rb_grl_fwd": (_int, [_p, _i64, _p, _i64, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _p,
                          _i64, _p, _p, _p, _p, _i64, _p, _p, _i64, _p]),
    "rb_probe_gemm_pattern": (_int, [_p, _i64, _i64, _p, _i64, _p]),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_derived_prototype_equals_pinned(name):
    table = (_lib.EXP_SIGNATURES if name == "rb_grl_fwd" else
             _lib.PROBE_SIGNATURES if name.startswith("rb_probe") else _lib.SIGNATURES)
    assert table[name] == PINNED[name]
    assert name != "rb_grl_fwd" or len(table[name][1]) == 25


@pytest.mark.parametrize("decl", ["int rb_x(long n);", "int rb_x(short n);",
                                  "int rb_x(rb_t job);", "int rb_x(struct rb_s job);",
                                  "int rb_x(int (*cb)(int));", "long rb_x(void);",
                                  "void rb_x(void);", "int rb_x(unsigned n);"])
def test_parser_rejects_what_it_cannot_type(decl):
    with pytest.raises(_lib.RecBLRNativeError, match="rb_x"):
        _lib.parse_header(decl)


def test_parser_skips_comments_typedefs_and_preprocessor_lines():
    text = """
    /* int rb_in_block_comment(void); calls rb_last_error_string() */
    // int rb_in_line_comment(void);
    #ifdef __cplusplus
    extern "C" {
    #endif
    #define RB_N 3
    typedef uint16_t rb_half;
    typedef struct { int64_t n; } rb_t;
    typedef struct {
      float* p;   /* int rb_in_struct(void); */
      int64_t n;
    } rb_u;
    const char* rb_msg(void);
    int64_t rb_f(const rb_u* jobs, int n, uint64_t seed, float p,
                 double lr, void* stream);
    #ifdef __cplusplus
    }
    #endif
    """
    assert _lib.parse_header(text) == {
        "rb_msg": (ctypes.c_char_p, []),
        "rb_f": (_i64, [_p, _int, _u64, _f32, _f64, _p]),
    }
    assert _lib.parse_header("typedef struct { int64_t n; } rb_t;") == {}


def test_argument_errors_are_reported_without_touching_the_gpu():
    lib = _lib.load()
    # null pointers are rejected before any HIP call
    rc = lib.rb_scan_fwd(None, None, None, 1, 1, 1, None)
    assert rc == _lib.RB_EINVAL
    assert b"null" in lib.rb_last_error_string()
    rc = lib.rb_conv_silu_fwd(1, 4, 1, 1, 1, 4, 1, 1, 4, 9, None, None)
    assert rc == _lib.RB_EINVAL
    assert b"K must be" in lib.rb_last_error_string()
    rc = lib.rb_gate_scan_fwd(1, 3, 1, 4, 1, 4, 1, 0, 0, 0, 1, 4, 1, 1, 1, 4, None, None)
    assert rc == _lib.RB_EINVAL   # rg row stride < 2H


# The seven recurrence entry points exist for fp32 and bf16 storage and share
# their checks: argument lists that pass every check (H = 4; non-null pointers
# are fake and never dereferenced), then one bad value each.
_P = 16
TWINS = {
    "rb_scan_fwd": dict(gates=_P, tokens=_P, states=_P, B=1, C=1, T=4, stream=None),
    "rb_scan_bwd": dict(gates=_P, states=_P, grad=_P, d_gates=_P, d_tokens=_P, B=1, C=1, T=4,
                        stream=None),
    "rb_conv_silu_fwd": dict(x=_P, x_rs=4, w=_P, bias=_P, xc=_P, xc_rs=4, B=1, L=1, H=4, K=4,
                             seq_offsets=None, stream=None),
    "rb_conv_silu_fwd_rows": dict(x=_P, x_rs=4, w=_P, bias=_P, xc=_P, xc_rs=4, B=8, H=4, K=4,
                                  row_pos=_P, stream=None),          # B: ntok
    "rb_conv_silu_bwd": dict(x=_P, x_rs=4, w=_P, bias=_P, g1=_P, g2=_P, dx=_P, dx_rs=4,
                             dw_part=_P, db_part=_P, B=1, L=1, H=4, K=4, seq_offsets=None,
                             stream=None),
    "rb_gate_scan_fwd": dict(rg=_P, rg_rs=8, xc=_P, xc_rs=4, z=_P, z_rs=4, lam=_P, gate_b=None,
                             h0=None, h0_bs=0, y=_P, y_rs=4, carries=_P, B=1, L=1, H=4,
                             seq_offsets=None, stream=None),
    "rb_gate_scan_bwd": dict(rg=_P, rg_rs=8, xc=_P, xc_rs=4, z=_P, z_rs=4, lam=_P, gate_b=None,
                             carries=_P, dy=_P, drg=_P, drg_rs=8, dxc=_P, dxc_rs=4, dz=_P,
                             dz_rs=4, part=_P, dh0_part=_P, B=1, L=1, H=4, seq_offsets=None,
                             stream=None),
}
_CONV = ("rb_conv_silu_fwd", "rb_conv_silu_fwd_rows", "rb_conv_silu_bwd")
_GATE = ("rb_gate_scan_fwd", "rb_gate_scan_bwd")
TWIN_CASES = (
    # a required pointer is null: the first, and the last one each check names
    [(fn, {next(iter(TWINS[fn])): None}, "null pointer") for fn in TWINS]
    + [("rb_scan_fwd", {"states": None}, "null pointer"),
       ("rb_scan_bwd", {"d_tokens": None}, "null pointer"),
       ("rb_conv_silu_fwd", {"xc": None}, "null pointer"),
       ("rb_conv_silu_fwd_rows", {"row_pos": None}, "null pointer"),
       ("rb_conv_silu_bwd", {"dw_part": None}, "null pointer"),
       ("rb_gate_scan_fwd", {"y": None}, "null pointer"),
       ("rb_gate_scan_bwd", {"dh0_part": None}, "null pointer")]
    + [(fn, {"K": k}, "kernel size K must be in [1, 8]") for fn in _CONV for k in (9, 0)]
    + [(fn, {"x_rs": 3}, "row stride < H") for fn in _CONV]
    + [(fn, {"rg_rs": 7}, "row stride too small") for fn in _GATE]      # rg holds 2H columns
    + [(fn, {"z_rs": 3}, "row stride too small") for fn in _GATE]
    + [(fn, {"B": 0}, "B, C, T must be positive") for fn in ("rb_scan_fwd", "rb_scan_bwd")]
    + [(fn, {"B": 0}, "B, L and H must be positive") for fn in _CONV + _GATE]
    + [("rb_gate_scan_fwd", {"h0": _P, "h0_bs": 1}, "h0 batch stride must be 0 or >= H")]
)


@pytest.mark.parametrize("fn,bad,what", TWIN_CASES,
                         ids=[f"{fn}-{'-'.join(f'{k}={v}' for k, v in bad.items())}"
                              for fn, bad, _ in TWIN_CASES])
def test_fp32_and_bf16_twins_reject_the_same_arguments(fn, bad, what):
    """Each recurrence entry point and its _bf16 twin fail the same check,
    before any launch (RB_EINVAL; a launch returns 0 or a positive hipError),
    with the same message behind their own name."""
    lib = _lib.load()
    assert set(bad) <= set(TWINS[fn])
    args = list({**TWINS[fn], **bad}.values())
    messages = []
    for name in (fn, fn + "_bf16"):
        assert len(args) == len(_lib.SIGNATURES[name][1])
        assert getattr(lib, name)(*args) == _lib.RB_EINVAL, name
        messages.append(lib.rb_last_error_string().decode())
    # the shape checks shared by the conv and gate entry points carry no name
    prefix = "" if what.startswith("B, L and H") else fn + ": "
    assert messages[0] == prefix + what
    assert messages[1] == (fn + "_bf16: " if prefix else "") + what


def test_row_conv_and_batched_split_argument_errors():
    """ABI 18/19 entry points validate before any HIP call."""
    lib = _lib.load()
    rc = lib.rb_conv_silu_fwd_rows(1, 4, 1, 1, 1, 4, 8, 4, 4, None, None)
    assert rc == _lib.RB_EINVAL and b"null" in lib.rb_last_error_string()
    rc = lib.rb_conv_silu_fwd_rows(1, 4, 1, 1, 1, 4, 8, 4, 9, 1, None)
    assert rc == _lib.RB_EINVAL and b"K must be" in lib.rb_last_error_string()
    from datamining_recblr_amd import kernels

    jobs = (kernels._SplitJob * 1)()
    jobs[0].W, jobs[0].ldw, jobs[0].C, jobs[0].R, jobs[0].transpose, jobs[0].Wf = 16, 40, 32, 40, 0, 16
    rc = lib.rb_gemm_h_split_weights(ctypes.addressof(jobs), 1, None)
    assert rc == _lib.RB_EINVAL and b"multiple of" in lib.rb_last_error_string()   # R % 16
    rc = lib.rb_gemm_h_split_weights(ctypes.addressof(jobs), 0, None)
    assert rc == _lib.RB_EINVAL
    rc = lib.rb_gemm_h_split_weights(ctypes.addressof(jobs), 33, None)
    assert rc == _lib.RB_EINVAL


def test_f16_item_ce_argument_errors():
    """ABI 24 entry points (the CE on split images) validate before any HIP call."""
    lib = _lib.load()
    rc = lib.rb_item_split_h(None, 4, 128, 16, 16, None, None)
    assert rc == _lib.RB_EINVAL and b"null" in lib.rb_last_error_string()
    rc = lib.rb_item_split_h(16, 4, 48, 16, 16, None, None)
    assert rc == _lib.RB_EINVAL and b"d must be" in lib.rb_last_error_string()
    rc = lib.rb_item_split_h(8, 4, 128, 16, 16, None, None)     # 8 is not 16-B aligned
    assert rc == _lib.RB_EINVAL and b"aligned" in lib.rb_last_error_string()
    rc = lib.rb_item_ce_fwd_h(16, None, 16, 16, 16, 4, 8, 128, 16, 16, 16, 1 << 20, None)
    assert rc == _lib.RB_EINVAL and b"exponent" in lib.rb_last_error_string()
    rc = lib.rb_item_ce_fwd_h(16, 16, 16, 16, 16, 4, 8, 100, 16, 16, 16, 1 << 20, None)
    assert rc == _lib.RB_EINVAL and b"d must be" in lib.rb_last_error_string()
    rc = lib.rb_item_ce_probs_h(16, 16, 16, 16, 16, 16, 16, 4, 8, 128, 0, 16, 7, None)
    assert rc == _lib.RB_EINVAL and b"ld < V" in lib.rb_last_error_string()


# The seven f16-pipe CE entry points (B = 4, V = 8, d = 128): argument lists
# that pass every check (the non-null pointers are fake and never
# dereferenced), then bad values; with two of them, the check that fires first.
_CE_OPS = dict(seq_img=_P, seq_exp=_P, item_img=_P, item_exp=_P, target=_P)
_CE_GRAD = dict(lse=_P, dloss=_P)
_CE_DIMS = dict(B=4, V=8, d=128)
_CE_FWD_OUT = dict(lse=_P, loss=_P, workspace=_P, workspace_bytes=1 << 20, stream=None)
_CE_P = dict(item_offset=0, probs=_P, ld=8)
_CE_PT = dict(probs_t=_P, ldt=4)
_CE_MAXES = dict(row_group_max=_P, item_group_max=_P, stream=None)
CE_H = {
    "rb_item_ce_fwd_h": {**_CE_OPS, **_CE_DIMS, **_CE_FWD_OUT},
    "rb_item_ce_fwd_h_rows": {**_CE_OPS, **_CE_DIMS, "inv_n": 0.5, "accumulate": 0, **_CE_FWD_OUT},
    "rb_item_ce_probs_h": {**_CE_OPS, **_CE_GRAD, **_CE_DIMS, **_CE_P, "stream": None},
    "rb_item_ce_probs_h_t": {**_CE_OPS, **_CE_GRAD, **_CE_DIMS, "item_offset": 0, **_CE_PT,
                             "group_max": _P, "stream": None},
    "rb_item_ce_probs_h_both": {**_CE_OPS, **_CE_GRAD, **_CE_DIMS, **_CE_P, **_CE_PT, **_CE_MAXES},
    "rb_item_ce_probs_h_rows": {**_CE_OPS, **_CE_GRAD, "inv_n": 0.5, **_CE_DIMS, **_CE_P,
                                "stream": None},
    "rb_item_ce_probs_h_both_rows": {**_CE_OPS, **_CE_GRAD, "inv_n": 0.5, **_CE_DIMS, **_CE_P,
                                     **_CE_PT, **_CE_MAXES},
}
_CE_SHARED = {"item scores (f16): null exponent pointer", "item scores: null pointer",
              "item scores: d must be 16, 32, 64, 128 or 256"}   # carry no entry point's name
_CE_LDT = "probs_t must be 16-B aligned with ldt >= B, ldt % 4 == 0"
_CE_INV_N = "inv_n must be in (0, 1]"
_CE_POINTERS = ("target", "lse", "loss", "dloss", "workspace", "probs", "probs_t", "group_max",
                "row_group_max", "item_group_max")
CE_H_CASES = (
    [(fn, {"seq_exp": None}, "item scores (f16): null exponent pointer") for fn in CE_H]
    + [(fn, {"item_img": None}, "item scores: null pointer") for fn in CE_H]
    + [(fn, {k: None}, "null pointer") for fn, ok in CE_H.items() for k in ok if k in _CE_POINTERS]
    + [(fn, {"ld": 7}, "ld < V") for fn, ok in CE_H.items() if "ld" in ok]
    + [(fn, bad, _CE_LDT) for fn, ok in CE_H.items() if "ldt" in ok
       for bad in ({"ldt": 3}, {"ldt": 6}, {"probs_t": 8})]      # < B; % 4; not 16-B aligned
    + [(fn, {"inv_n": v}, _CE_INV_N) for fn, ok in CE_H.items() if "inv_n" in ok
       for v in (0.0, 1.5, -0.5, float("nan"))]
    + [("rb_item_ce_fwd_h_rows", {"accumulate": 2}, "accumulate must be 0 or 1"),
       ("rb_item_ce_fwd_h_rows", {"accumulate": -1}, "accumulate must be 0 or 1")]
    # two bad values: operands, then null pointers, inv_n, accumulate / ld, ldt
    + [(fn, {"d": 100, "target": None}, "item scores: d must be 16, 32, 64, 128 or 256")
       for fn in CE_H]
    + [(fn, {"lse": None, "inv_n": 0.0}, "null pointer") for fn, ok in CE_H.items() if "inv_n" in ok]
    + [("rb_item_ce_fwd_h_rows", {"inv_n": 1.5, "accumulate": 2}, _CE_INV_N),
       ("rb_item_ce_probs_h_rows", {"inv_n": 1.5, "ld": 7}, _CE_INV_N),
       ("rb_item_ce_probs_h_both_rows", {"inv_n": 1.5, "ld": 7, "ldt": 3}, _CE_INV_N),
       ("rb_item_ce_probs_h_both_rows", {"ld": 7, "ldt": 3}, "ld < V"),
       ("rb_item_ce_probs_h_both", {"ld": 7, "ldt": 3}, "ld < V"),
       ("rb_item_ce_probs_h_both", {"dloss": None, "ld": 7}, "null pointer"),
       ("rb_item_ce_probs_h_t", {"group_max": None, "ldt": 3}, "null pointer")]
)


@pytest.mark.parametrize("fn,bad,what", CE_H_CASES,
                         ids=[f"{fn}-{'-'.join(f'{k}={v}' for k, v in bad.items())}"
                              for fn, bad, _ in CE_H_CASES])
def test_f16_item_ce_entry_points_refuse_with_their_own_message(fn, bad, what):
    """Each of the seven refuses before any launch (RB_EINVAL) with exactly the
    message behind its own name, and with the earliest failing check's."""
    lib = _lib.load()
    assert set(bad) <= set(CE_H[fn])
    args = list({**CE_H[fn], **bad}.values())
    assert len(args) == len({**_lib.SIGNATURES, **_lib.DENSE_SIGNATURES}[fn][1])
    assert getattr(lib, fn)(*args) == _lib.RB_EINVAL
    want = what if what in _CE_SHARED else f"{fn}: {what}"
    assert lib.rb_last_error_string().decode() == want


def test_probe_library_is_separate_and_exports_its_header():
    """bench.py's measurement aids live in their own library
    (probes/recblr_probe.h, lib/libdmrecblr_probe.so): the product library
    exports none of them, the probe library exports exactly its header's."""
    hdr = os.path.join(os.path.dirname(_lib.__file__), "probes", "recblr_probe.h")
    text = re.sub(r"/\*.*?\*/", "", open(hdr).read(), flags=re.S)
    names = re.findall(r"\b(rb_[a-z0-9_]+)\s*\(", text)
    assert set(names) == set(_lib.PROBE_SIGNATURES)
    assert _lib.PROBE_SIGNATURES["rb_probe_last_error_string"] == (ctypes.c_char_p, [])
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert not hasattr(raw, n), n
    probe = _lib.load_probe()
    for n in names:
        assert hasattr(probe, n), n
    # argument errors are reported without touching the GPU
    try:
        _lib.call_probe("rb_probe_gemm_pattern", None, 1, 4, None, 4, None)
    except _lib.RecBLRNativeError as e:
        assert "null pointer" in str(e)
    else:
        raise AssertionError("null pointers accepted")


def test_tn_weight_gradient_rejects_row_chunks_of_2_gib():
    """rb_gemm_tn_h addresses a row chunk with 32-bit offsets through a buffer
    descriptor: a chunk spanning 2 GiB of an operand is an argument error
    naming the limit (checked before any HIP call), never a silent wrap."""
    lib = _lib.load()
    M, N, K = 1 << 22, 128, 128
    # 8 splits of 2^22 rows: 2^19-row chunks; at a 2^13-float row stride of dY
    # a chunk spans 2^19 x 32 KiB = 16 GiB
    rc = lib.rb_gemm_tn_h(16, 1 << 13, 16, K, M, N, K, 16, 16, 16, 8, None)
    assert rc == _lib.RB_EINVAL and b"2 GiB" in lib.rb_last_error_string()


def test_experimental_library_is_separate_and_exports_its_header():
    """The opt-in fused GatedRecurrentLayer kernels (RECBLR_FUSED_GRL*) live
    in their own library (experimental/recblr_exp.h, lib/libdmrecblr_exp.so):
    the product library exports none of them, the experimental library
    exactly its header's, at the product's ABI version; argument errors are
    reported without touching the GPU."""
    hdr = os.path.join(os.path.dirname(_lib.__file__), "experimental", "recblr_exp.h")
    text = re.sub(r"/\*.*?\*/", "", open(hdr).read(), flags=re.S)
    names = re.findall(r"\b(rb_[a-z0-9_]+)\s*\(", text)
    assert set(names) == set(_lib.EXP_SIGNATURES)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert not hasattr(raw, n), n
    exp = _lib.load_exp()
    assert _lib.ABI_VERSION == _lib.load().rb_version() == exp.rb_exp_version()
    try:
        _lib.call_exp("rb_grl_fwd", *[0 if t is ctypes.c_int64 else None
                                      for t in _lib.EXP_SIGNATURES["rb_grl_fwd"][1]])
    except _lib.RecBLRNativeError as e:
        assert "null pointer" in str(e)
    else:
        raise AssertionError("null pointers accepted")
