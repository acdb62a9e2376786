"""CPU: the kernel symbol of every forward / dgrad convolution launch, as the library's routing reports it
(sgg_conv2d_nhwc_fwd_symbol / _dgrad_symbol: the launch's own validation and route, no GPU), against the routing table
tests/golden/conv_symbols.json.

The table was generated at the commit before the routes existed, from the hand-written Python restatement of the four dispatch
ladders that lib.py then carried (HipKernels.conv_symbol): both directions; precisions 0, 1, 2, 3, 4, 6; w_split_layout 0 .. 4 on
every channel pair of {32, 64, 128, 256, 512} the layout's applicability predicate accepts; with and without pre-split weights, tile
statistics, LN prologue and pre-split source where the entry point accepts the combination; the band kernel on both sides of
cdiv(M, 224) * (N / 256) = 128 | 129 and cdiv(M, 224) * (N / 128) = 256 | 257; every encoder launch (trunk._plan) at
bench.CONFIGS[1], [3], [4] and at 221 px, forward-only and with-backward passes, in every precision and under the routing options.
The C dispatch agreed with that restatement on every row.  Rows that share direction, precision, layout and grid form a group; a
row adds the channels, the presence flags and operand_format (Ho, Wo and the pads follow from SAME padding), then the index into
`symbols`."""
import ctypes
import json
import os

import sgg_amd  # noqa: F401
from sgg_amd import build, lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_symbols.json")


def _query(L, group, row):
    """group / row: the table's group_fields / row_fields; Ho, Wo and the pads are those of SAME padding (as HipKernels._conv_dims
    passes them), KH = KW = K."""
    direction, precision, layout, K, stride, B, Hi, Wi = group
    Cin, Cout, ws, stats, ln, fmt = row[:6]
    Ho, pad_t, _ = lib.same_pads(Hi, K, stride)
    Wo, pad_l, _ = lib.same_pads(Wi, K, stride)
    dims = (B, Hi, Wi, Cin, Ho, Wo, Cout, K, K, stride, pad_t, pad_l, precision, layout, ws)
    buf = ctypes.create_string_buffer(128)
    if direction == "fwd":
        rc = L.sgg_conv2d_nhwc_fwd_symbol(*dims, stats, ln, fmt, buf, len(buf))
    else:       # (dgrad: no tile statistics, no LN prologue)
        assert direction == "dgrad" and (stats, ln) == (0, 0)
        rc = L.sgg_conv2d_nhwc_dgrad_symbol(*dims, fmt, buf, len(buf))
    return rc, buf.value.decode()


def test_reported_symbols_equal_the_routing_table():
    L = lib.load_library(build.build())
    table = json.load(open(GOLDEN))
    assert table["group_fields"] == ["dir", "precision", "w_split_layout", "K", "stride", "B", "Hi", "Wi"]
    assert table["row_fields"] == ["Cin", "Cout", "w_split", "tile_stats", "ln", "operand_format", "symbol_index"]
    groups, symbols = table["groups"], table["symbols"]
    cases = [(g[:8], r) for g in groups for r in g[8]]
    assert len(cases) == 4868 and len({(tuple(g), tuple(r[:6])) for g, r in cases}) == 4868
    assert {g[0] for g, _ in cases} == {"fwd", "dgrad"} and {g[1] for g, _ in cases} == {0, 1, 2, 3, 4, 6} and {g[2] for g, _ in cases} == {0, 1, 2, 3, 4}
    assert {r[6] for _, r in cases} == set(range(len(symbols)))
    wrong = []
    for g, r in cases:
        rc, sym = _query(L, g, r)
        if rc != 0 or sym != symbols[r[6]]:
            wrong.append((g, r, symbols[r[6]], rc, sym if rc == 0 else L.sgg_last_error().decode()))
    assert not wrong, "%d of %d rows differ, first: %s" % (len(wrong), len(cases), wrong[:5])


def test_query_refuses_what_the_launch_refuses():
    """Same validation, same message (sgg_last_error) as the launch entry point."""
    L = lib.load_library(build.build())
    buf = ctypes.create_string_buffer(128)
    dims = (2, 16, 16, 64, 16, 16, 128, 3, 3, 1, 1, 1)
    cases = [
        (L.sgg_conv2d_nhwc_fwd_symbol, dims + (2, 4, 0, 0, 0, 0), "w_split_layout 1 / 4 needs"),            # layout 4 without pre-split weights
        (L.sgg_conv2d_nhwc_fwd_symbol, dims + (4, 1, 1, 0, 1, 0), "two-piece modes (2, 3) only"),           # LN prologue in a one-piece mode
        (L.sgg_conv2d_nhwc_fwd_symbol, dims + (3, 1, 1, 0, 0, 1), "a pre-split (S16) x needs"),             # pre-split x with bf16 pieces
        (L.sgg_conv2d_nhwc_fwd_symbol, dims + (5, 0, 0, 0, 0, 0), "precision must be"),
        (L.sgg_conv2d_nhwc_fwd_symbol, dims + (2, 0, 0, 0, 0, 33 << 8), "operand_format"),                  # more CUs than an XCD has
        (L.sgg_conv2d_nhwc_dgrad_symbol, dims + (2, 2, 1, 0), "w_split_layout 2 needs 5x5 stride 2"),
        (L.sgg_conv2d_nhwc_dgrad_symbol, (2, 16, 16, 64, 16, 16, 64, 3, 3, 1, 1, 1, 2, 4, 1, 0), "w_split_layout 4 needs"),    # 64 columns, f32 dy
    ]
    for fn, args, text in cases:
        assert fn(*args, buf, len(buf)) == -1, args
        assert text in L.sgg_last_error().decode(), (args, L.sgg_last_error().decode())
    assert L.sgg_conv2d_nhwc_fwd_symbol(*dims, 2, 1, 1, 0, 0, 0, buf, 8) == -1      # buffer too small
    assert L.sgg_conv2d_nhwc_fwd_symbol(2, 16, 16, 3, 16, 16, 32, 3, 3, 1, 1, 1, 2, 0, 0, 1, 0, 0, buf, len(buf)) == 0
    assert buf.value == b"conv_c3_fwd_kernel"
