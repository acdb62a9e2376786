"""CPU: the routing of every filter-gradient launch, as the library reports it (sgg_conv2d_nhwc_wgrad_symbol: the launch's own
validation and route, no GPU), against the routing table tests/golden/wgrad_routes.json.

How the table was made.  A shape is (K, stride, B, Hi, Wi, Cin, Cout); Ho, Wo and the pads are those of SAME padding.  Shapes: every
live conv layer of the encoder (both networks share it) at bench.CONFIGS[1] / [3] (64 x 224 px), [4] (32 x 448 px) and at 221 px (its
224 px canvas and the plain odd grid); 3x3 stride 1 and 5x5 stride 2 on every channel pair of {32, 64, 128, 256, 512} over dy grids
that 8x8 blocks tile (16x16), that only row bands serve (14x14, 7x60; 28x28 among the layers) and that neither serves (12x120);
Cin = 3 (accepted and refused); per-tap shapes with one pixel split (dw written directly) and with several; odd x grids under
stride 2; a 4x4 kernel; a 96-channel tile.  Rows per shape: precisions 0, 1, 2, 3, 4, 6 x (algo 0 plain, with operand_format 3,
with an LN prologue; algo 1 plain), in precision 2 also operand_format 1 and 2, the LN prologue under every operand_format and algo 1
with pre-split operands / with LN; the channel pairs above 128 take (plain, operand_format 3, LN) with algo 0 in precisions 2 and 3.

Columns of the PARENT (the commit named in the file, before the route existed), generated against a library built from it with that
commit's lib.py: per shape sgg_conv2d_nhwc_wgrad_workspace_bytes, the sgg_conv2d_nhwc_wgrad_resident code in every precision, and
[wgrad_resident, ln_prologue_ok] of an object made with HipKernels.__new__ that carries the library and the default options, at
conv_precision 2 and 3; per row the timing label by the condition HipKernels.conv_wgrad then spelled out (x_s16 and dy_s16 and no LN
and precision 2 and algo 0 and resident code 2 -> conv_wgrad_dma; Cin == 3 -> conv_c3_wgrad; else conv_wgrad).  A label exists only
where the launch is accepted: a refused launch raises before its label is used.  For every refused row the parent's launch entry
point, called with dummy pointers and a workspace declared large enough, returned SGG_ERR_ARG with the very message recorded here.

Columns of the library with the route: the symbols, the exact workspace bytes and the message of a refused row are what
sgg_conv2d_nhwc_wgrad_symbol reported (a whole number of dW slabs; 27 x 32 floats each for Cin = 3): recorded from this library, so
they pin its routing rather than check it against an independent reference - a kernel trace on the GPU does that
(scripts/wgrad_route_ab.py --traces, profiles/wgrad_route_trace.log)."""
import ctypes
import json
import os

import sgg_amd  # noqa: F401
from sgg_amd import build, lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_routes.json")
PRECISIONS = (0, 1, 2, 3, 4, 6)
_cache = {}


def _table():
    """[(shape dims with Ho, Wo, pads; shape columns; row; rc; symbols | message; workspace bytes)], queried once."""
    if not _cache:
        L = lib.load_library(build.build())
        t = json.load(open(GOLDEN))
        assert t["row_fields"] == ["precision", "algo", "ln", "operand_format", "label_index", "symbols_index", "workspace_bytes", "message_index"]
        cases = []
        for K, stride, B, Hi, Wi, Cin, Cout, upper, codes, meth, rows in t["shapes"]:
            Ho, pad_t, _ = lib.same_pads(Hi, K, stride)
            Wo, pad_l, _ = lib.same_pads(Wi, K, stride)
            dims = (B, Hi, Wi, Cin, Ho, Wo, Cout, K, K, stride, pad_t, pad_l)
            for row in rows:
                buf, ws = ctypes.create_string_buffer(256), ctypes.c_size_t(0)
                rc = L.sgg_conv2d_nhwc_wgrad_symbol(*dims, *row[:4], ctypes.addressof(ws), buf, len(buf))
                cases.append((dims, (upper, codes, meth), row, rc, buf.value.decode() if rc == 0 else L.sgg_last_error().decode(), ws.value))
        _cache.update(L=L, t=t, cases=cases)
    return _cache["L"], _cache["t"], _cache["cases"]


def _family(symbols):
    return symbols.split("<")[0]


def test_table_covers_what_it_claims():
    _, t, cases = _table()
    assert len(t["parent"]) == 40 and len(cases) == 4302
    assert {c[2][0] for c in cases} == set(PRECISIONS) and {c[2][1] for c in cases} == {0, 1}
    assert {(c[2][2], c[2][3]) for c in cases} == {(ln, fmt) for ln in (0, 1) for fmt in (0, 1, 2, 3)}
    ok = [c for c in cases if c[3] == 0]
    assert {_family(c[4]) for c in ok} == {"conv_c3_wgrad_kernel", "conv_wgrad_kernel", "conv_wgrad_tr_kernel", "conv_wgrad_halo3_kernel",
                                           "conv_wgrad_dma_kernel", "conv_wgrad_dma_rb_kernel"}
    assert {c[4].split(">")[0].split(",")[7] for c in ok if _family(c[4]) == "conv_wgrad_halo3_kernel"} == {"0", "1"}      # GEO: blocks, row bands
    assert {c[4].count(";") for c in ok} == {0, 3}                                    # one kernel, or the four tap classes of 5x5 stride 2
    taps = [c for c in ok if _family(c[4]) in ("conv_wgrad_kernel", "conv_wgrad_tr_kernel")]
    assert any(c[5] == 0 for c in taps) and any(c[5] > 0 for c in taps)               # nsplit == 1 (dw written directly) and > 1
    assert {c[2][5] for c in ok} == set(range(len(t["symbols"])))
    assert {c[2][7] for c in cases if c[3] != 0} == set(range(len(t["messages"])))


def test_query_reproduces_the_table():
    """Symbols, exact workspace bytes; a refused row is refused with the recorded message."""
    _, t, cases = _table()
    wrong = []
    for dims, _, row, rc, text, ws in cases:
        if row[5] >= 0:
            per = 4 * (27 * 32 if dims[3] == 3 else dims[7] * dims[8] * dims[3] * dims[6])
            good = rc == 0 and text == t["symbols"][row[5]] and ws == row[6] and ws % per == 0      # (whole dW slabs)
        else:
            good = rc == -1 and text == t["messages"][row[7]]
        if not good:
            wrong.append((dims, row, rc, text, ws))
    assert not wrong, "%d of %d rows differ, first: %s" % (len(wrong), len(cases), wrong[:5])


def test_parent_columns_are_reproduced():
    """Workspace upper bound, resident code, timing label, HipKernels.wgrad_resident / ln_prologue_ok: as before the route."""
    L, t, cases = _table()
    K = lib.HipKernels.__new__(lib.HipKernels)
    K.lib = L
    for key, val in lib.DEFAULT_OPTIONS.items():
        setattr(K, key, val)
    wrong = []
    for Kk, stride, B, Hi, Wi, Cin, Cout, upper, codes, meth, _ in t["shapes"]:
        Ho, Wo = lib.same_pads(Hi, Kk, stride)[0], lib.same_pads(Wi, Kk, stride)[0]
        got = [L.sgg_conv2d_nhwc_wgrad_workspace_bytes(B, Hi, Wi, Cin, Ho, Wo, Cout, Kk, Kk),
               [L.sgg_conv2d_nhwc_wgrad_resident(B, Ho, Wo, Cin, Cout, Kk, Kk, stride, p) for p in PRECISIONS], []]
        for precision in (2, 3):
            K.conv_precision = precision
            got[2].append([int(K.wgrad_resident(B, Ho, Wo, Cin, Cout, Kk, stride)), int(bool(K.ln_prologue_ok(Kk, stride, Hi, Wi, Cin, Cout)))])
        if got != [upper, codes, meth]:
            wrong.append(((Kk, stride, B, Hi, Wi, Cin, Cout), got, [upper, codes, meth]))
    assert not wrong, "%d shapes differ, first: %s" % (len(wrong), wrong[:5])
    labels = [(c[0], c[2]) for c in cases if c[3] == 0 and next(lab for pre, lab in lib.WGRAD_LABELS if c[4].startswith(pre)) != t["labels"][c[2][4]]]
    assert not labels, labels[:5]
    assert all(c[2][4] == -1 for c in cases if c[3] != 0)


def test_families_sit_where_the_parent_put_them():
    _, t, cases = _table()
    for dims, (upper, codes, _), row, rc, text, ws in cases:
        precision, algo, ln, fmt = row[:4]
        code = codes[PRECISIONS.index(precision)]
        fam = _family(text) if rc == 0 else None
        dma = fam in ("conv_wgrad_dma_kernel", "conv_wgrad_dma_rb_kernel")
        # (the resident code knows the dy grid only; an odd x grid under stride 2 - 221 px - is not twice the dy grid: there the launch
        # with pre-split operands is refused, before the route as after it)
        aligned = dims[1] == dims[4] * dims[9] and dims[2] == dims[5] * dims[9]
        assert dma == (code == 2 and fmt == 3 and not ln and precision == 2 and algo == 0 and aligned), (dims, row, text)
        assert fam != "conv_wgrad_halo3_kernel" or code >= 1, (dims, row, text)
        assert rc != 0 or ws <= upper, (dims, row, ws, upper)


def test_launch_refuses_with_the_message_of_the_query():
    """The launch entry point on every refused row (dummy pointers, a workspace declared large enough): it returns before any HIP call,
    with the query's message - they share one validation."""
    L, t, cases = _table()
    mem = ctypes.create_string_buffer(64)
    p = ctypes.addressof(mem)
    refused = [c for c in cases if c[3] != 0]
    assert len(refused) == 2265
    for dims, _, row, rc, text, _ in refused:
        ln = p if row[2] else None
        assert L.sgg_conv2d_nhwc_wgrad(p, p, p, *dims, row[0], row[1], p, p, ln, ln, ln, row[3], p, 1 << 40, None) == -1, (dims, row)
        assert L.sgg_last_error().decode() == text, (dims, row)
    # what the query alone checks, and what only the launch can see
    buf = ctypes.create_string_buffer(256)
    dims = (2, 16, 16, 64, 16, 16, 64, 3, 3, 1, 1, 1)
    assert L.sgg_conv2d_nhwc_wgrad_symbol(*dims, 2, 0, 0, 0, None, buf, 64) == -1 and "at least 256 bytes" in L.sgg_last_error().decode()
    assert L.sgg_conv2d_nhwc_wgrad_symbol(*dims, 2, 0, 0, 0, None, buf, 256) == 0 and buf.value == b"conv_wgrad_halo3_kernel<2,2,true,true,3,3,false,0,false>"
    assert L.sgg_conv2d_nhwc_wgrad(p, p, p, *dims, 2, 0, None, None, None, None, None, 0, p, 1 << 40, None) == -1
    assert "need the amax words" in L.sgg_last_error().decode()
    assert L.sgg_conv2d_nhwc_wgrad(p, p, p, *dims, 2, 0, p, p, p, None, None, 0, p, 1 << 40, None) == -1
    assert "needs stats, gamma and beta" in L.sgg_last_error().decode()
    assert L.sgg_conv2d_nhwc_wgrad(p, p, p, *dims, 2, 0, p, p, None, None, None, 0, p, 8, None) == -3      # SGG_ERR_WORKSPACE: no launch either
