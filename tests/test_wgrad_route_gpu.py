"""-m gpu: the workspace a filter-gradient launch needs is exactly what sgg_conv2d_nhwc_wgrad_symbol reports for it - one shape per
kernel family of the route (csrc/conv_halo.h: WgradRoute).

  * with a workspace of exactly the reported bytes, followed by a 4 KB canary inside the same allocation, dw is bit for bit what a
    roomy workspace gives, and the canary stays intact;
  * declaring one byte less on the same (real, large enough) buffer is refused with SGG_ERR_WORKSPACE before anything is launched.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = [
    # family (the kernel the query must report), (B, H, W, Cin, Cout, k, stride), precision, algo, operand_format
    ("conv_c3_wgrad_kernel", (2, 16, 32, 3, 32, 3, 1), 2, 0, 0),
    ("conv_wgrad_kernel", (3, 12, 30, 32, 64, 3, 1), 2, 1, 0),              # per-tap, two pixel splits
    ("conv_wgrad_tr_kernel", (3, 12, 30, 128, 128, 3, 1), 2, 1, 0),         # per-tap transposed
    ("conv_wgrad_halo3_kernel", (2, 32, 32, 32, 64, 5, 2), 2, 0, 0),        # halo-resident on 8x8 blocks, the four tap classes
    ("conv_wgrad_halo3_kernel", (3, 20, 20, 64, 64, 3, 1), 3, 0, 0),        # halo-resident on row bands
    ("conv_wgrad_dma_kernel", (2, 16, 16, 64, 128, 3, 1), 2, 0, 3),         # LDS-DMA on 8x8 blocks
    ("conv_wgrad_dma_rb_kernel", (2, 28, 28, 128, 64, 5, 2), 2, 0, 3),      # LDS-DMA on row bands, the four tap classes
]
CANARY = 4096


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s" % (c[0], "x".join(map(str, c[1]))))
def test_launch_runs_in_exactly_the_reported_workspace(hip, case):
    from sgg_amd.lib import same_pads, _p
    family, (B, H, W, Ci, Co, k, s), precision, algo, fmt = case
    (Ho, pt, _), (Wo, pl, _) = same_pads(H, k, s), same_pads(W, k, s)
    dims = (B, H, W, Ci, Ho, Wo, Co, k, k, s, pt, pl)
    L = hip.lib
    buf, need = ctypes.create_string_buffer(256), ctypes.c_size_t(0)
    assert L.sgg_conv2d_nhwc_wgrad_symbol(*dims, precision, algo, 0, fmt, ctypes.addressof(need), buf, len(buf)) == 0, L.sgg_last_error()
    symbols = buf.value.decode().split(";")
    assert {sym.split("<")[0] for sym in symbols} == {family} and len(symbols) == (4 if s == 2 else 1), symbols
    if family == "conv_wgrad_halo3_kernel":
        assert symbols[0].split(">")[0].split(",")[7] == ("1" if H % (8 * s) else "0")         # GEO: 8x8 blocks / row bands
    need = need.value
    assert 0 < need <= L.sgg_conv2d_nhwc_wgrad_workspace_bytes(*dims[:9]) and need % 16 == 0

    gen = torch.Generator().manual_seed(11)
    x = torch.randn((B, H, W, Ci), generator=gen).cuda()
    dy = torch.randn((B, Ho, Wo, Co), generator=gen).cuda()
    am = torch.zeros(2, device="cuda")
    hip.absmax(x, am[0:1])
    hip.absmax(dy, am[1:2])
    if fmt & 1:
        hip.presplit16(x, x, am[0:1])
    if fmt & 2:
        hip.presplit16(dy, dy, am[1:2])

    def launch(ws, declared):
        dw = torch.full((k, k, Ci, Co), float("nan"), device="cuda")
        rc = L.sgg_conv2d_nhwc_wgrad(_p(x), _p(dy), _p(dw), *dims, precision, algo, _p(am[0:1]), _p(am[1:2]), None, None, None, fmt, _p(ws),
                                     declared, hip._stream())
        return rc, dw

    roomy = torch.zeros(2 * need + (1 << 20), dtype=torch.uint8, device="cuda")
    rc, want = launch(roomy, roomy.numel())
    assert rc == 0 and bool(torch.isfinite(want).all()), L.sgg_last_error()

    tight = torch.empty(need + CANARY, dtype=torch.uint8, device="cuda")
    tight[:need] = 0xff              # (NaN patterns where a slab is not written)
    tight[need:] = 0x5a
    rc, got = launch(tight, need)
    assert rc == 0, L.sgg_last_error()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert bool((tight[need:] == 0x5a).all()), "the launch wrote past the workspace it reported"

    rc, untouched = launch(tight, need - 1)
    assert rc == -3 and b"workspace too small" in L.sgg_last_error()           # SGG_ERR_WORKSPACE
    assert bool(torch.isnan(untouched).all()) and bool((tight[need:] == 0x5a).all())
