"""The cases of tests/test_conv_routes_gpu.py: one fp64-checked launch for every convolution kernel instance the routing tables
know - the 137 filter-gradient kernels of tests/golden/wgrad_routes.json and the 78 forward / dgrad symbols of
tests/golden/conv_symbols.json - each row NAMED for the kernels it must reach.  Importable without torch and without a GPU:
tests/test_conv_routes_cpu.py asks the library's route queries (sgg_conv2d_nhwc_wgrad_symbol / _fwd_symbol / _dgrad_symbol) for every
row and checks that the union of the rows' kernels is the union of the tables' - an instance the library can route to and no row
reaches fails there, on the CPU.

Filter gradients: (B, H, W, Cin, Cout, k, stride, precision, algo, ln, operand_format, symbols).  Ho, Wo and the pads are those of SAME
padding; a 5x5 stride-2 launch on the resident kernels starts the four tap-parity classes (Q below).  Shapes: the smallest at which the
kernel's loops still take more than one trip -
  per-tap tiles (algo 1)   3 x 12 x 30: 1080 pixels = two pixel splits of 544 (a multiple of 32, not of 64: the 64-pixel-slab instances
                           end on a ragged slab) that cross image boundaries; 256 channels: more than one channel tile per launch
  fall-through (algo 0)    1 x 4 x 60 at 64 channels: a row band would need 184 patch slots (limit 176), so the resident kernels refuse;
                           240 pixels: one slab, dw written directly, no workspace
  8x8 blocks               dy grids of 8 x 8 to 24 x 16 over two or three images: 4 to 18 blocks per launch
  row bands                12 x 20 in bands of 5, 5 and 2 rows; 14 x 14 in 8-row bands with a ragged second band; 20 x 20 in bands of 5
  LN prologue              x is the producing layer's pre-LayerNorm output (ln = 1)
  operand_format           bit 0: x pre-split, bit 1: dy pre-split; 3 in precision 2 without LN: the LDS-DMA kernels

Forward / dgrad: (direction, precision, w_split_layout, k, stride, B, H, W, Cin, Cout, w_split, tile_stats, ln, operand_format, symbol),
one row per symbol: the table's smallest row for it (ties: the row that also asks for tile statistics), except
  conv_c3_fwd_kernel   the table holds it at the benchmark's image sizes only; 3 x 13 x 45 has ragged tiles on both edges
  tile_stats           0 where sgg_conv2d_nhwc_fwd_tile_stats is 0 (the native f32 kernels emit none)
The eight-wave conv_s2_kernel<...,8> needs more than 128 (band, 256-column) work items: B = 65 at 512 output columns.
"""


def Q(pattern):
    """The four tap-parity classes of a 5x5 stride-2 launch, in launch order."""
    return ";".join(pattern % cls for cls in ("2,2", "2,3", "3,2", "3,3"))


H3 = "conv_wgrad_halo3_kernel<%s>"
PT = "conv_wgrad_kernel<%s>"

# ---- the per-tap kernels: nine channel tiles x four precision forms, and the transposed kernel of the 128 x 128 tile --------------
_PER_TAP = {  # (Cin, Cout) -> template arguments in front of the precision form
    (32, 32): "32,32,32,32", (32, 64): "32,64,32,32", (32, 128): "32,128,32,32",
    (64, 32): "64,32,32,32", (64, 64): "64,64,32,32", (64, 128): "64,128,32,64",
    (128, 32): "128,32,32,32", (128, 64): "128,64,64,32", (128, 128): "128,128,64,64",
}
_FORMS = {0: "0,false", 2: "2,true", 3: "2,false", 6: "3,false"}      # precision -> (pieces, fp16)
_TR = {2: "conv_wgrad_tr_kernel<2,true>", 3: "conv_wgrad_tr_kernel<2,false>", 6: "conv_wgrad_tr_kernel<3,false>"}


def _per_tap(ci, co, p):
    if min(ci, co) >= 128 and p:
        return _TR[p]
    return PT % (_PER_TAP[(min(ci, 128), min(co, 128))] + "," + _FORMS[p])


WGRAD_PER_TAP = [(3, 12, 30, ci, co, 3, 1, p, 1, 0, 0, _per_tap(ci, co, p)) for (ci, co) in _PER_TAP for p in (0, 2, 3, 6)] + \
                [(3, 12, 30, 256, 256, 3, 1, p, 1, 0, 0, _per_tap(256, 256, p)) for p in (0, 2, 3, 6)] + \
                [(1, 4, 60, 64, 64, 3, 1, p, 0, 0, 0, _per_tap(64, 64, p)) for p in (0, 2, 3, 6)]

# ---- the resident kernels ---------------------------------------------------------------------------------------------------------
WGRAD_RESIDENT = [
    (2, 10, 10, 3, 32, 3, 1, 0, 0, 0, 0, "conv_c3_wgrad_kernel<false>"),
    # 5x5 stride 2 on 8x8 blocks: 32 -> 32 (conv1_3; 18 blocks), 32 -> 64 (4 blocks), 64 -> 128 (6 blocks); one- and two-piece forms
    (3, 48, 32, 32, 32, 5, 2, 1, 0, 0, 0, Q(H3 % "1,1,true,true,%s,false,0,true")),
    (3, 48, 32, 32, 32, 5, 2, 2, 0, 0, 0, Q(H3 % "1,1,true,true,%s,false,0,false")),
    (3, 48, 32, 32, 32, 5, 2, 3, 0, 0, 0, Q(H3 % "1,1,false,true,%s,false,0,false")),
    (3, 48, 32, 32, 32, 5, 2, 4, 0, 0, 0, Q(H3 % "1,1,false,true,%s,false,0,true")),
    (2, 32, 16, 32, 64, 5, 2, 1, 0, 0, 0, Q(H3 % "1,2,true,false,%s,false,0,true")),
    (2, 32, 16, 32, 64, 5, 2, 2, 0, 0, 0, Q(H3 % "1,2,true,false,%s,false,0,false")),
    (2, 32, 16, 32, 64, 5, 2, 3, 0, 0, 0, Q(H3 % "1,2,false,false,%s,false,0,false")),
    (2, 32, 16, 32, 64, 5, 2, 4, 0, 0, 0, Q(H3 % "1,2,false,false,%s,false,0,true")),
    (3, 16, 32, 64, 128, 5, 2, 1, 0, 0, 0, Q(H3 % "2,2,true,true,%s,false,0,true")),
    (3, 16, 32, 64, 128, 5, 2, 2, 0, 0, 0, Q(H3 % "2,2,true,true,%s,false,0,false")),
    (3, 16, 32, 64, 128, 5, 2, 3, 0, 0, 0, Q(H3 % "2,2,false,true,%s,false,0,false")),
    (3, 16, 32, 64, 128, 5, 2, 4, 0, 0, 0, Q(H3 % "2,2,false,true,%s,false,0,true")),
    # 5x5 stride 2 in row bands: a 12 x 20 dy grid in bands of 5, 5 and 2 rows
    (2, 24, 40, 64, 64, 5, 2, 1, 0, 0, 0, Q(H3 % "2,2,true,true,%s,false,1,true")),
    (2, 24, 40, 64, 64, 5, 2, 2, 0, 0, 0, Q(H3 % "2,2,true,true,%s,false,1,false")),
    (2, 24, 40, 64, 64, 5, 2, 3, 0, 0, 0, Q(H3 % "2,2,false,true,%s,false,1,false")),
    (2, 24, 40, 64, 64, 5, 2, 4, 0, 0, 0, Q(H3 % "2,2,false,true,%s,false,1,true")),
    # the LN prologue in the stride-2 tap classes: conv1_3, then the forms no older case reached (conv2_5 is <2,2,true,true,..,true,0,false>)
    (3, 48, 32, 32, 32, 5, 2, 2, 0, 1, 0, Q(H3 % "1,1,true,true,%s,true,0,false")),
    (3, 48, 32, 32, 32, 5, 2, 3, 0, 1, 0, Q(H3 % "1,1,false,true,%s,true,0,false")),
    (2, 32, 32, 32, 64, 5, 2, 2, 0, 1, 0, Q(H3 % "1,2,true,false,%s,true,0,false")),
    (2, 32, 32, 32, 64, 5, 2, 3, 0, 1, 0, Q(H3 % "1,2,false,false,%s,true,0,false")),
    (2, 32, 32, 64, 64, 5, 2, 2, 0, 1, 0, Q(H3 % "2,2,true,true,%s,true,0,false")),
    (2, 32, 32, 64, 64, 5, 2, 3, 0, 1, 0, Q(H3 % "2,2,false,true,%s,true,0,false")),
    # 3x3 stride 1 (the 3,3 class alone): plain, with the LN prologue, with one pre-split operand (the register-staged path)
    (2, 16, 24, 32, 32, 3, 1, 2, 0, 0, 0, H3 % "1,1,true,true,3,3,false,0,false"),
    (2, 16, 24, 32, 32, 3, 1, 2, 0, 1, 0, H3 % "1,1,true,true,3,3,true,0,false"),
    (2, 16, 16, 32, 64, 3, 1, 1, 0, 0, 0, H3 % "1,2,true,false,3,3,false,0,true"),
    (2, 16, 16, 32, 64, 3, 1, 2, 0, 0, 0, H3 % "1,2,true,false,3,3,false,0,false"),
    (2, 16, 16, 32, 64, 3, 1, 3, 0, 0, 0, H3 % "1,2,false,false,3,3,false,0,false"),
    (2, 16, 16, 32, 64, 3, 1, 4, 0, 0, 0, H3 % "1,2,false,false,3,3,false,0,true"),
    (2, 16, 16, 32, 64, 3, 1, 2, 0, 1, 0, H3 % "1,2,true,false,3,3,true,0,false"),
    (3, 8, 16, 64, 64, 3, 1, 2, 0, 1, 0, H3 % "2,2,true,true,3,3,true,0,false"),
    (3, 8, 16, 64, 64, 3, 1, 2, 0, 0, 2, H3 % "2,2,true,true,3,3,false,0,false"),
    (1, 8, 16, 128, 64, 3, 1, 2, 0, 0, 1, H3 % "2,2,true,true,3,3,false,0,false"),
    # LDS-DMA: 64 and 128 output columns on 8x8 blocks (3x3, and the four classes of 5x5 stride 2), row bands
    (3, 24, 16, 128, 128, 3, 1, 2, 0, 0, 3, "conv_wgrad_dma_kernel<4,3,3>"),
    (2, 16, 48, 64, 128, 5, 2, 2, 0, 0, 3, Q("conv_wgrad_dma_kernel<4,%s>")),
    (2, 32, 32, 64, 64, 5, 2, 2, 0, 0, 3, Q("conv_wgrad_dma_kernel<2,%s>")),
    (2, 20, 20, 64, 64, 3, 1, 2, 0, 0, 3, "conv_wgrad_dma_rb_kernel<3,3>"),
    (2, 28, 28, 128, 64, 5, 2, 2, 0, 0, 3, Q("conv_wgrad_dma_rb_kernel<%s>")),
]

WGRAD_CASES = WGRAD_PER_TAP + WGRAD_RESIDENT

# ---- forward / dgrad: one row per symbol of the table -------------------------------------------------------------------------------
GB = "conv_gather_bf16s_kernel<%s>"
HK = "conv_halo3_kernel<%s>"
PC = "conv_halo3_pc_kernel<%s>"
S2 = "conv_s2_kernel<%s>"
FWD_DGRAD_CASES = [
    ("fwd", 2, 0, 3, 1, 3, 13, 45, 3, 32, 0, 1, 0, 0, "conv_c3_fwd_kernel"),
    # gather kernels (w_split_layout 0): native f32, then pieces 2 | 3, pre-split weights or not, fp16 or bf16
    ("fwd", 0, 0, 3, 1, 2, 16, 16, 32, 128, 0, 0, 0, 0, "conv_gather3_kernel<128,128,2,2,32>"),
    ("fwd", 0, 0, 3, 1, 2, 16, 16, 32, 32, 0, 0, 0, 0, "conv_gather3_kernel<256,32,4,1,32>"),
    ("fwd", 0, 0, 3, 1, 2, 16, 16, 32, 64, 0, 0, 0, 0, "conv_gather_kernel<256,64,4,1>"),
    ("fwd", 3, 0, 3, 1, 2, 16, 16, 32, 128, 0, 1, 0, 0, GB % "128,128,2,2,2,false,false,32"),
    ("fwd", 2, 0, 3, 1, 2, 16, 16, 32, 128, 0, 1, 0, 0, GB % "128,128,2,2,2,false,true,32"),
    ("fwd", 3, 0, 3, 1, 2, 16, 16, 32, 128, 1, 1, 0, 0, GB % "128,128,2,2,2,true,false,32"),
    ("fwd", 2, 0, 3, 1, 2, 16, 16, 32, 128, 1, 1, 0, 0, GB % "128,128,2,2,2,true,true,32"),
    ("fwd", 6, 0, 3, 1, 2, 16, 16, 32, 128, 0, 1, 0, 0, GB % "128,128,2,2,3,false,false,32"),
    ("fwd", 6, 0, 3, 1, 2, 16, 16, 32, 128, 1, 1, 0, 0, GB % "128,128,2,2,3,true,false,32"),
    ("fwd", 3, 0, 3, 1, 2, 16, 16, 32, 32, 0, 1, 0, 0, GB % "256,32,4,1,2,false,false,32"),
    ("fwd", 2, 0, 3, 1, 2, 16, 16, 32, 32, 0, 1, 0, 0, GB % "256,32,4,1,2,false,true,32"),
    ("fwd", 3, 0, 3, 1, 2, 16, 16, 32, 32, 1, 1, 0, 0, GB % "256,32,4,1,2,true,false,32"),
    ("fwd", 2, 0, 3, 1, 2, 16, 16, 32, 32, 1, 1, 0, 0, GB % "256,32,4,1,2,true,true,32"),
    ("fwd", 6, 0, 3, 1, 2, 16, 16, 32, 32, 0, 1, 0, 0, GB % "256,32,4,1,3,false,false,32"),
    ("fwd", 6, 0, 3, 1, 2, 16, 16, 32, 32, 1, 1, 0, 0, GB % "256,32,4,1,3,true,false,32"),
    ("fwd", 3, 0, 3, 1, 2, 16, 16, 32, 64, 0, 1, 0, 0, GB % "256,64,4,1,2,false,false,32"),
    ("fwd", 2, 0, 3, 1, 2, 16, 16, 32, 64, 0, 1, 0, 0, GB % "256,64,4,1,2,false,true,32"),
    ("fwd", 3, 0, 3, 1, 2, 16, 16, 32, 64, 1, 1, 0, 0, GB % "256,64,4,1,2,true,false,32"),
    ("fwd", 2, 0, 3, 1, 2, 16, 16, 32, 64, 1, 1, 0, 0, GB % "256,64,4,1,2,true,true,32"),
    ("fwd", 6, 0, 3, 1, 2, 16, 16, 32, 64, 0, 1, 0, 0, GB % "256,64,4,1,3,false,false,32"),
    ("fwd", 6, 0, 3, 1, 2, 16, 16, 32, 64, 1, 1, 0, 0, GB % "256,64,4,1,3,true,false,32"),
    # halo-resident 3x3 (layout 1) and conv1_3's dgrad through the space-to-depth view (layout 3): 128-, 32- and 64-column tilings
    ("fwd", 3, 1, 3, 1, 2, 16, 24, 64, 128, 1, 1, 0, 0, HK % "2,128,2,2,false,true,false,false,false,1"),
    ("fwd", 4, 1, 3, 1, 2, 16, 24, 64, 128, 1, 1, 0, 0, HK % "2,128,2,2,false,true,false,false,true,1"),
    ("fwd", 3, 1, 3, 1, 2, 16, 24, 64, 128, 1, 1, 1, 0, HK % "2,128,2,2,false,true,false,true,false,1"),
    ("dgrad", 3, 3, 5, 2, 2, 32, 32, 32, 32, 1, 0, 0, 0, HK % "2,128,2,2,false,true,true,false,false,1"),
    ("dgrad", 4, 3, 5, 2, 2, 32, 32, 32, 32, 1, 0, 0, 0, HK % "2,128,2,2,false,true,true,false,true,1"),
    ("fwd", 3, 1, 3, 1, 2, 16, 24, 32, 128, 1, 1, 1, 0, HK % "2,128,2,2,false,true,true,true,false,1"),
    ("fwd", 2, 1, 3, 1, 2, 16, 24, 64, 128, 1, 1, 0, 0, HK % "2,128,2,2,true,true,false,false,false,1"),
    ("fwd", 1, 1, 3, 1, 2, 16, 24, 64, 128, 1, 1, 0, 0, HK % "2,128,2,2,true,true,false,false,true,1"),
    ("fwd", 2, 1, 3, 1, 2, 16, 24, 64, 128, 1, 1, 1, 0, HK % "2,128,2,2,true,true,false,true,false,1"),
    ("dgrad", 2, 3, 5, 2, 2, 32, 32, 32, 32, 1, 0, 0, 0, HK % "2,128,2,2,true,true,true,false,false,1"),
    ("dgrad", 1, 3, 5, 2, 2, 32, 32, 32, 32, 1, 0, 0, 0, HK % "2,128,2,2,true,true,true,false,true,1"),
    ("fwd", 2, 1, 3, 1, 2, 16, 24, 32, 128, 1, 1, 1, 0, HK % "2,128,2,2,true,true,true,true,false,1"),
    ("fwd", 3, 1, 3, 1, 2, 16, 24, 64, 32, 1, 1, 0, 0, HK % "2,32,2,1,false,true,false,false,false,1"),
    ("fwd", 4, 1, 3, 1, 2, 16, 24, 64, 32, 1, 1, 0, 0, HK % "2,32,2,1,false,true,false,false,true,1"),
    ("fwd", 3, 1, 3, 1, 2, 16, 24, 64, 32, 1, 1, 1, 0, HK % "2,32,2,1,false,true,false,true,false,1"),
    ("fwd", 3, 1, 3, 1, 2, 16, 24, 32, 32, 1, 1, 0, 0, HK % "2,32,2,1,false,true,true,false,false,1"),
    ("fwd", 4, 1, 3, 1, 2, 16, 24, 32, 32, 1, 1, 0, 0, HK % "2,32,2,1,false,true,true,false,true,1"),
    ("fwd", 3, 1, 3, 1, 2, 16, 24, 32, 32, 1, 1, 1, 0, HK % "2,32,2,1,false,true,true,true,false,1"),
    ("fwd", 2, 1, 3, 1, 2, 16, 24, 64, 32, 1, 1, 0, 0, HK % "2,32,2,1,true,true,false,false,false,1"),
    ("fwd", 1, 1, 3, 1, 2, 16, 24, 64, 32, 1, 1, 0, 0, HK % "2,32,2,1,true,true,false,false,true,1"),
    ("fwd", 2, 1, 3, 1, 2, 16, 24, 64, 32, 1, 1, 1, 0, HK % "2,32,2,1,true,true,false,true,false,1"),
    ("fwd", 2, 1, 3, 1, 2, 16, 24, 32, 32, 1, 1, 0, 0, HK % "2,32,2,1,true,true,true,false,false,1"),
    ("fwd", 1, 1, 3, 1, 2, 16, 24, 32, 32, 1, 1, 0, 0, HK % "2,32,2,1,true,true,true,false,true,1"),
    ("fwd", 2, 1, 3, 1, 2, 16, 24, 32, 32, 1, 1, 1, 0, HK % "2,32,2,1,true,true,true,true,false,1"),
    ("fwd", 3, 1, 3, 1, 2, 16, 24, 64, 64, 1, 1, 0, 0, HK % "2,64,2,2,false,true,false,false,false,1"),
    ("fwd", 4, 1, 3, 1, 2, 16, 24, 64, 64, 1, 1, 0, 0, HK % "2,64,2,2,false,true,false,false,true,1"),
    ("fwd", 3, 1, 3, 1, 2, 16, 24, 64, 64, 1, 1, 1, 0, HK % "2,64,2,2,false,true,false,true,false,1"),
    ("fwd", 3, 1, 3, 1, 2, 16, 24, 32, 64, 1, 1, 0, 0, HK % "2,64,2,2,false,true,true,false,false,1"),
    ("fwd", 4, 1, 3, 1, 2, 16, 24, 32, 64, 1, 1, 0, 0, HK % "2,64,2,2,false,true,true,false,true,1"),
    ("fwd", 3, 1, 3, 1, 2, 16, 24, 32, 64, 1, 1, 1, 0, HK % "2,64,2,2,false,true,true,true,false,1"),
    ("fwd", 2, 1, 3, 1, 2, 16, 24, 64, 64, 1, 1, 0, 0, HK % "2,64,2,2,true,true,false,false,false,1"),
    ("fwd", 1, 1, 3, 1, 2, 16, 24, 64, 64, 1, 1, 0, 0, HK % "2,64,2,2,true,true,false,false,true,1"),
    ("fwd", 2, 1, 3, 1, 2, 16, 24, 64, 64, 1, 1, 1, 0, HK % "2,64,2,2,true,true,false,true,false,1"),
    ("fwd", 2, 1, 3, 1, 2, 16, 24, 32, 64, 1, 1, 0, 0, HK % "2,64,2,2,true,true,true,false,false,1"),
    ("fwd", 1, 1, 3, 1, 2, 16, 24, 32, 64, 1, 1, 0, 0, HK % "2,64,2,2,true,true,true,false,true,1"),
    ("fwd", 2, 1, 3, 1, 2, 16, 24, 32, 64, 1, 1, 1, 0, HK % "2,64,2,2,true,true,true,true,false,1"),
    # producer / consumer 3x3 (layout 4): bf16 | fp16, LN prologue, pre-split source in the two- and the four-block form
    ("fwd", 3, 4, 3, 1, 2, 16, 24, 64, 128, 1, 1, 0, 0, PC % "false,false,false,2"),
    ("fwd", 3, 4, 3, 1, 2, 16, 24, 64, 128, 1, 1, 1, 0, PC % "false,true,false,2"),
    ("fwd", 2, 4, 3, 1, 2, 16, 24, 64, 128, 1, 1, 0, 0, PC % "true,false,false,2"),
    ("fwd", 2, 4, 3, 1, 2, 16, 24, 64, 128, 1, 1, 0, 1, PC % "true,false,true,2"),
    ("fwd", 2, 4, 3, 1, 2, 16, 24, 64, 64, 1, 1, 0, 1, PC % "true,false,true,4"),
    ("fwd", 2, 4, 3, 1, 2, 16, 24, 64, 128, 1, 1, 1, 0, PC % "true,true,false,2"),
    # band-resident 5x5 stride 2 (layout 2): a 14 x 16 grid = one band of 224 positions per image
    ("fwd", 3, 2, 5, 2, 2, 28, 32, 32, 128, 1, 1, 0, 0, S2 % "false,false,7,false,false,false,4"),
    ("fwd", 3, 2, 5, 2, 2, 28, 32, 32, 128, 1, 1, 1, 0, S2 % "false,false,7,false,true,false,4"),
    ("fwd", 4, 2, 5, 2, 2, 28, 32, 32, 128, 1, 1, 0, 0, S2 % "false,false,7,true,false,false,4"),
    ("fwd", 2, 2, 5, 2, 2, 28, 32, 32, 128, 1, 1, 0, 0, S2 % "false,true,7,false,false,false,4"),
    ("fwd", 2, 2, 5, 2, 2, 28, 32, 32, 128, 1, 1, 0, 1, S2 % "false,true,7,false,false,true,4"),
    ("fwd", 2, 2, 5, 2, 65, 28, 32, 32, 512, 1, 1, 0, 1, S2 % "false,true,7,false,false,true,8"),
    ("fwd", 2, 2, 5, 2, 2, 28, 32, 32, 128, 1, 1, 1, 0, S2 % "false,true,7,false,true,false,4"),
    ("fwd", 1, 2, 5, 2, 2, 28, 32, 32, 128, 1, 1, 0, 0, S2 % "false,true,7,true,false,false,4"),
    ("dgrad", 3, 2, 5, 2, 2, 28, 32, 128, 32, 1, 0, 0, 0, S2 % "true,false,7,false,false,false,4"),
    ("dgrad", 4, 2, 5, 2, 2, 28, 32, 128, 32, 1, 0, 0, 0, S2 % "true,false,7,true,false,false,4"),
    ("dgrad", 2, 2, 5, 2, 2, 28, 32, 128, 32, 1, 0, 0, 0, S2 % "true,true,7,false,false,false,4"),
    ("dgrad", 2, 2, 5, 2, 2, 28, 32, 128, 32, 1, 0, 0, 1, S2 % "true,true,7,false,false,true,4"),
    ("dgrad", 2, 2, 5, 2, 65, 28, 32, 512, 32, 1, 0, 0, 1, S2 % "true,true,7,false,false,true,8"),
    ("dgrad", 1, 2, 5, 2, 2, 28, 32, 128, 32, 1, 0, 0, 0, S2 % "true,true,7,true,false,false,4"),
]


def same_pads(in_size, k, s):
    """TF SAME padding: (out, before, after) - as sgg_amd.lib.same_pads (restated: this module imports nothing)."""
    out = -(-in_size // s)
    total = max((out - 1) * s + k - in_size, 0)
    return out, total // 2, total - total // 2


def conv_dims(B, H, W, Ci, Co, k, s):
    """The twelve leading scalars of the convolution entry points and of their route queries."""
    (Ho, pt, _), (Wo, pl, _) = same_pads(H, k, s), same_pads(W, k, s)
    return (B, H, W, Ci, Ho, Wo, Co, k, k, s, pt, pl)


def wgrad_query(L, case):
    """(symbols, exact workspace bytes) of a WGRAD_CASES row, from the library (L = the loaded library)."""
    import ctypes
    buf, need = ctypes.create_string_buffer(256), ctypes.c_size_t(0)
    rc = L.sgg_conv2d_nhwc_wgrad_symbol(*conv_dims(*case[:7]), *case[7:11], ctypes.addressof(need), buf, len(buf))
    assert rc == 0, (case, L.sgg_last_error())
    return buf.value.decode(), need.value


def fwd_dgrad_query(L, case):
    """The symbol of a FWD_DGRAD_CASES row, from the library."""
    import ctypes
    direction, precision, layout, k, s, B, H, W, Ci, Co, w_split, stats, ln, fmt = case[:14]
    buf = ctypes.create_string_buffer(128)
    dims = conv_dims(B, H, W, Ci, Co, k, s)
    if direction == "fwd":
        rc = L.sgg_conv2d_nhwc_fwd_symbol(*dims, precision, layout, w_split, stats, ln, fmt, buf, len(buf))
    else:
        assert direction == "dgrad" and (stats, ln) == (0, 0), case
        rc = L.sgg_conv2d_nhwc_dgrad_symbol(*dims, precision, layout, w_split, fmt, buf, len(buf))
    assert rc == 0, (case, L.sgg_last_error())
    return buf.value.decode()


def case_symbols(L):
    """({filter-gradient kernels}, {forward / dgrad symbols}) the library's route queries report over the two lists; asserts that
    each case reaches the kernels it is named for."""
    wgrad, fd = set(), set()
    for case in WGRAD_CASES:
        got = wgrad_query(L, case)[0]
        assert got == case[11], (case[:11], got, case[11])
        wgrad.update(got.split(";"))
    for case in FWD_DGRAD_CASES:
        got = fwd_dgrad_query(L, case)
        assert got == case[14], (case[:14], got, case[14])
        fd.add(got)
    return wgrad, fd
