"""The cases of tests/test_head_routes_gpu.py: every kernel route of the head GEMM (csrc/gemm.hip) and of the attention step
(csrc/head.hip), each NAMED for the kernels it must reach.  Importable without a GPU: tests/test_head_routes_cpu.py asks the
library's route queries for every case and checks that the kernels of every head launch of the benchmark configurations
(tests/head_shapes.py) appear among them - a route the step takes and no case reaches fails there, on the CPU.

GEMM case: (mode, M, N, K, form, kernels).  mode 0 = NN, 1 = NT, 2 = TN.  Forms of the operands A and B (C always lands in a
column slice of a wider NaN-filled buffer):
    plain      contiguous, 16-byte aligned
    ld+4       leading dimension = width + 4
    off1       base pointer one float past a 16-byte boundary, leading dimension a multiple of 4: the scalar load path, chosen
               by the pointer alone
    tail2      contiguous dimension = 2 mod 4 inside a leading dimension rounded up to a multiple of 4: the vector path with a
               tail of 2 (K for A, and for B in NT; the M / N tails of the tiled kernels)
    bias+acc   NN with bias and accumulate together
"""
WK = "gemm_wk_kernel<%d,%s,%d>"
NN, NT, TN = 0, 1, 2
TILES = {NN: "gemm_kernel<false,false>", NT: "gemm_kernel<false,true>", TN: "gemm_kernel<true,false>"}
NARROW, WIDE = ";gemm_slab_reduce_kernel", ";gemm_slab_reduce_wide_kernel"


def wk(tm, mode):
    return WK % (tm, "true" if mode == NT else "false", 2 if tm >= 4 else 4)


# ---- every instance of the split-K-in-a-workgroup kernel, the slab routes next to them, the edges of its applicability ---------
GEMM_INSTANCES = [
    # TM 2: the M = 64 gates product and the decoder / W_c products of the batch-64 step; ragged M and N with scalar loads and a K tail of 3
    (NN, 64, 2048, 1324, "plain", wk(2, NN)),
    (NN, 128, 1000, 512, "plain", wk(2, NN)),
    (NN, 49, 2045, 131, "plain", wk(2, NN)),
    (NT, 49, 2045, 131, "plain", wk(2, NT)),
    # TM 4: the critic's gates dgrad; ragged
    (NT, 192, 1324, 2048, "plain", wk(4, NT)),
    (NN, 178, 1321, 514, "plain", wk(4, NN)),
    (NT, 178, 1321, 514, "plain", wk(4, NT)),
    # TM 6, just under the M in 65 .. 128, N * K >= 2^21 exclusion; the slab kernels on and above it
    (NN, 128, 2048, 1023, "plain", wk(6, NN)),
    (NT, 256, 1324, 2048, "plain", wk(6, NT)),                      # the gates dgrad of a critic at batch 128
    (NN, 128, 2048, 1024, "plain", TILES[NN] + NARROW),
    (NT, 65, 2048, 1024, "plain", TILES[NT] + NARROW),
    # TM 1 edges: one k group per wave; M = 512 | 513; N = 16 | 15; K = 8192 | 8193
    (NN, 17, 16, 128, "plain", wk(1, NN)),
    (NT, 17, 16, 128, "plain", wk(1, NT)),
    (NN, 512, 16, 128, "plain", wk(1, NN)),
    (NN, 513, 16, 128, "plain", TILES[NN] + NARROW),
    (NT, 512, 16, 128, "plain", wk(1, NT)),
    (NT, 513, 16, 128, "plain", TILES[NT] + NARROW),
    (NN, 16, 16, 128, "plain", wk(1, NN)),
    (NN, 16, 15, 128, "plain", TILES[NN] + NARROW),
    (NT, 16, 16, 128, "plain", wk(1, NT)),
    (NT, 16, 15, 128, "plain", TILES[NT] + NARROW),
    (NN, 16, 16, 8192, "plain", wk(1, NN)),
    (NN, 16, 16, 8193, "plain", TILES[NN] + WIDE),
    (NT, 16, 16, 8192, "plain", wk(1, NT)),
    (NT, 16, 16, 8193, "plain", TILES[NT] + WIDE),
]

# ---- operand forms through a wk, a direct, a narrow-reduce and a wide-reduce route in all three modes (TN has no wk route) -----
# route -> mode -> ((M, N, K) of ld+4 / off1 / bias+acc, (M, N, K) of tail2)
# tail2 is K = 130 inside ld = 132 wherever a route exists at that K: the direct route then needs 64 tiles (512 x 512), the wide
# reduce needs 16 slabs and so K = 8706 inside ld = 8708; in TN the contiguous dimensions are M and N, so those carry the tail
_FORM_SHAPES = {
    "wk": {NN: ((24, 48, 512), (24, 48, 130)), NT: ((24, 48, 512), (24, 48, 130))},
    "direct": {NN: ((70, 132, 100), (512, 512, 130)), NT: ((70, 132, 100), (512, 512, 130)), TN: ((72, 132, 100), (70, 130, 100))},
    "narrow": {NN: ((516, 16, 132), (516, 16, 130)), NT: ((516, 16, 132), (516, 16, 130)), TN: ((40, 48, 132), (42, 50, 132))},
    "wide": {NN: ((8, 16, 8704), (8, 16, 8706)), NT: ((8, 16, 8704), (8, 16, 8706)), TN: ((8, 16, 8704), (10, 18, 8704))},
}


def _route_kernels(route, mode):
    return {"wk": wk(1, mode), "direct": TILES[mode], "narrow": TILES[mode] + NARROW, "wide": TILES[mode] + WIDE}[route]


GEMM_FORMS = []
for _route, _modes in _FORM_SHAPES.items():
    for _mode, (_base, _tail) in _modes.items():
        GEMM_FORMS += [(_mode,) + _base + ("ld+4", _route_kernels(_route, _mode)), (_mode,) + _base + ("off1", _route_kernels(_route, _mode)),
                       (_mode,) + _tail + ("tail2", _route_kernels(_route, _mode))]
        if _mode == NN:
            GEMM_FORMS.append((_mode,) + _base + ("bias+acc", _route_kernels(_route, _mode)))

GEMM_CASES = GEMM_INSTANCES + GEMM_FORMS

# ---- attention forward, per-row kernel: (B, N = R / B, L, C), float and dual --------------------------------------------------
#   (2, 1, 16, 256)     one workgroup per row, one 256-channel pass
#   (2, 2, 196, 768)    C % 512 != 0: one workgroup per row, three passes
#   (2, 1, 16, 1024)    two workgroups per row, two passes each
#   (256, 1, 16, 512)   R = 256: one workgroup per row, two passes (a critic at batch 128 has R = 384)
#   (86, 3, 16, 512)    R = 258 over three rows per image
#   (1, 1, 8000, 256)   dual only: 72 KB of dynamic LDS, beyond the default limit of a launch
ATTN_FWD_CASES = [(B, N, L, C, dual) for (B, N, L, C) in [(2, 1, 16, 256), (2, 2, 196, 768), (2, 1, 16, 1024), (256, 1, 16, 512), (86, 3, 16, 512)]
                  for dual in (False, True)] + [(1, 1, 8000, 256, True)]

SPLIT = "attn_step_bwd_ctx_kernel<%s>;attn_step_bwd_softmax_kernel<%s>"
FUSED = "attn_step_bwd_kernel<%s>"
# ---- attention backward: (B, npass, L, C, dual, kernels); each runs with accumulate on and off --------------------------------
ATTN_BWD_CASES = [(B, npass, L, C, dual, (SPLIT if split else FUSED).replace("%s", "Dual" if dual else "float"))
                  for (B, npass, L, C, split, duals) in [
                      (64, 3, 196, 512, True, (False, True)),       # the batch-64 critic step: ls = 8
                      (2, 4, 64, 256, True, (False, True)),         # L = 64, the lower edge; npass = ATTN_MAX_PASS
                      (1, 2, 2048, 256, True, (False, True)),       # L = 2048, the upper edge: dp[8] of the softmax kernel exactly full
                      (200, 1, 100, 256, True, (False, True)),      # ls = 2
                      (2, 2, 2049, 256, False, (False,)),           # fused beyond L = 2048: its l += 256 loops iterate
                      (2, 1, 2049, 256, False, (True,)),            # (dual with one row per image: 34 KB of dynamic LDS)
                      (256, 1, 70, 256, False, (False, True)),      # fused from B = 256
                      (1, 1, 10000, 256, False, (False,)),          # 81 KB of dynamic LDS, beyond the default limit of a launch
                  ] for dual in duals]


def case_symbols(L):
    """{kernels} the library's route queries (L = the loaded library) report over all cases; asserts that each case reaches the
    route it is named for."""
    import ctypes
    buf, syms = ctypes.create_string_buffer(96), set()
    for mode, M, N, K, form, kernels in GEMM_CASES:
        assert L.sgg_gemm_skinny_symbol(mode, M, N, K, None, buf, len(buf)) == 0, L.sgg_last_error()
        assert buf.value.decode() == kernels, ((mode, M, N, K, form), buf.value.decode(), kernels)
        syms.add(kernels)
    for B, N, Lc, C, dual in ATTN_FWD_CASES:
        assert L.sgg_attn_step_fwd_symbol(B * N, B, Lc, C, int(dual), buf, len(buf)) == 0, L.sgg_last_error()
        assert buf.value.decode() == "attn_step_fwd_kernel<%s>" % ("Dual" if dual else "float"), (B, N, Lc, C, dual)
        syms.add(buf.value.decode())
    for B, npass, Lc, C, dual, kernels in ATTN_BWD_CASES:
        assert L.sgg_attn_step_bwd_symbol(B * npass, B, Lc, C, int(dual), buf, len(buf)) == 0, L.sgg_last_error()
        assert buf.value.decode() == kernels, ((B, npass, Lc, C, dual), buf.value.decode(), kernels)
        syms.add(kernels)
    return syms
