"""How the loss, fill and pooling kernels cut their work into workgroups: a Python restatement of the launch arithmetic of
csrc/misc.hip (onehot, interpolate, gp_fwd, gp_bwd, wgan_losses, argmax_rows, fill, absmax) and of the two spatial-mean kernels of
csrc/head.hip, and the cases of tests/test_loss_geometry_gpu.py (test infrastructure, importable without a GPU).

Every case carries the property it exists for (trips of a loop, a second trip of a capped grid, waves that hold data, a tail
launch, ...).  tests/test_loss_cases_cpu.py recomputes each property from the arithmetic below and compares the constants with the
sources: a change of a cap or of a block size then names the cases that left the path they were built for.
"""
from collections import namedtuple

BLOCK = 256            # threads of every kernel here but onehot's / fill's tail launch (blockDim.x, the `i += 256` loops, block_sum_256)
WAVE = 64              # lanes: one wave per row in argmax_rows, four waves per workgroup
GRID_FOR_CAP = 4096    # grid_for (csrc/sgg_common.h)
EW_CAP = 64            # workgroups per sample of interpolate and gp_bwd (grid-stride loop behind it)
ABSMAX_CAP = 1024      # workgroups of absmax
FILL4_MIN = 4096       # sgg_fill: 16-byte stores from this length on, if the pointer is 16-byte aligned
SM_GY = 16             # spatial_mean_bwd: blockIdx.y slices over L
SM_CW = 128            # spatial_mean_fwd: channels per workgroup (32 lanes x float4)
SM_RG = 8              # spatial_mean_fwd: row groups over L (256 threads / 32 lanes)
ARGMAX_ROWS = 4        # argmax_rows: rows per workgroup (BLOCK / WAVE)


def cdiv(a, b):
    return -(-a // b)


def grid_for(n, block=BLOCK):
    return max(1, min(cdiv(n, block), GRID_FOR_CAP))


# ---- interpolate, gp_bwd: grid (min(grid_for(n), 64), B), `i += gridDim.x * 256` ---------------------------------------------------
def ew_grid(n):
    return min(grid_for(n), EW_CAP)


def ew_trips(n):
    """the most trips a thread of the grid-stride loop makes"""
    return cdiv(n, ew_grid(n) * BLOCK)


# ---- gp_fwd, wgan_losses: one workgroup per row / one workgroup, `i += 256`, block_sum_256 over four waves ---------------------------
def block_trips(n):
    return cdiv(n, BLOCK)


def waves_with_data(n):
    """waves of the workgroup whose lanes read at least one element"""
    return min(BLOCK // WAVE, cdiv(n, WAVE))


# ---- absmax: float4 body on min(grid_for(n / 4 + 1), 1024) workgroups, the n & 3 tail in workgroup 0 ---------------------------------
def absmax_grid(n):
    return min(grid_for(n // 4 + 1), ABSMAX_CAP)


def absmax_trips(n):
    return cdiv(n // 4, absmax_grid(n) * BLOCK)


# ---- fill ------------------------------------------------------------------------------------------------------------------------
def fill_path(n, aligned):
    """(path, workgroups of the first launch, most trips of a thread, elements of the tail launch)"""
    if n >= FILL4_MIN and aligned:
        g = grid_for(n // 4)
        return ("fill4+tail" if n & 3 else "fill4", g, cdiv(n // 4, g * BLOCK), n & 3)
    g = grid_for(n)
    return ("scalar", g, cdiv(n, g * BLOCK), 0)


# ---- spatial means ---------------------------------------------------------------------------------------------------------------
def sm_fwd_grid(B, C):
    return (B, cdiv(C, SM_CW))


def sm_fwd_rows(L):
    """rows each of the 8 row groups sums"""
    return [len(range(rg, L, SM_RG)) for rg in range(SM_RG)]


def sm_bwd_gy(L):
    return min(L, SM_GY)


def sm_bwd_rows(L):
    """rows each blockIdx.y slice writes"""
    gy = sm_bwd_gy(L)
    return [len(range(y, L, gy)) for y in range(gy)]


# ---- argmax_rows -----------------------------------------------------------------------------------------------------------------
def argmax_grid(rows):
    return cdiv(rows, ARGMAX_ROWS)


def argmax_idle_waves(rows):
    """waves of the last workgroup that leave through `row >= rows`"""
    return argmax_grid(rows) * ARGMAX_ROWS - rows


def argmax_trips(V):
    return cdiv(V, WAVE)


# ---- path signatures: two shapes with equal signatures run the same branches and loop forms ---------------------------------------
def many(t):
    return min(t, 2)            # 0, 1, "2 or more" trips


def sig_ew(n):
    return (many(ew_trips(n)), ew_grid(n) == EW_CAP)


def sig_block(n):
    return (many(block_trips(n)), waves_with_data(n))


def sig_argmax(rows, V, ld):
    return (many(argmax_trips(V)), V % WAVE != 0, argmax_idle_waves(rows) > 0, ld > V)


def sig_sm_fwd(L, C):
    r = sm_fwd_rows(L)
    return (many(max(r)), min(r) == 0, len(set(r)) > 1, C % SM_CW != 0)


def sig_sm_bwd_y(L):            # (the loop over L and the one over C are independent)
    r = sm_bwd_rows(L)
    return (sm_bwd_gy(L) == SM_GY, many(max(r)), len(set(r)) > 1)


def sig_sm_bwd_c(C):
    return (many(cdiv(C, BLOCK)), C % BLOCK != 0)


def sig_fill(n, aligned):
    """(kernel of the first launch, its trips); the tail launch does not depend on either"""
    p = fill_path(n, aligned)
    return (p[0].split("+")[0], many(p[2]))


# ---- the cases -------------------------------------------------------------------------------------------------------------------
# fill: n, element offset of the start from a 16-byte boundary, path, most trips per thread.  The last case is the only one whose
# float4 grid reaches grid_for's cap: the gradient arenas (34 M floats) are filled by that grid-stride loop.
FillCase = namedtuple("FillCase", "n offset path trips")
FILL_CASES = [
    FillCase(1, 0, "scalar", 1), FillCase(3, 0, "scalar", 1), FillCase(4095, 0, "scalar", 1),
    FillCase(4096, 0, "fill4", 1), FillCase(4097, 0, "fill4+tail", 1), FillCase(4099, 0, "fill4+tail", 1),
    FillCase(65536 + 3, 0, "fill4+tail", 1),
    FillCase(4096, 1, "scalar", 1), FillCase(4097, 1, "scalar", 1), FillCase(4099, 1, "scalar", 1), FillCase(65536 + 3, 1, "scalar", 1),
    FillCase(4 * (GRID_FOR_CAP * BLOCK + 1) + 3, 0, "fill4+tail", 2),
]
FILL_VALUES = ["0.0", "-1/192", "-0.0", "nan"]

# absmax: n, workgroups, most float4 trips per thread, tail elements
AbsmaxCase = namedtuple("AbsmaxCase", "n grid trips tail")
ABSMAX_CASES = [
    AbsmaxCase(1, 1, 0, 1), AbsmaxCase(3, 1, 0, 3), AbsmaxCase(4, 1, 1, 0), AbsmaxCase(5, 1, 1, 1), AbsmaxCase(1027, 2, 1, 3),
    AbsmaxCase(4 * BLOCK * ABSMAX_CAP + 7, ABSMAX_CAP, 2, 3),       # the capped grid strides
]

# onehot: rows (as [B, T] labels), V, trips of the `i += 256` loop
OnehotCase = namedtuple("OnehotCase", "B T V trips")
ONEHOT_CASES = [OnehotCase(64, 3, 50, 1), OnehotCase(64, 3, 256, 1), OnehotCase(64, 3, 257, 2), OnehotCase(64, 3, 1000, 4)]

# interpolate: B, T, V (n = T * V per sample), workgroups per sample, whether the grid-stride loop makes a second trip
EwCase = namedtuple("EwCase", "B n grid second_grid_trip")
INTERP_V = [50, 1000, 5461, 5462]
INTERP_CASES = [EwCase(5, 150, 1, False), EwCase(5, 3000, 12, False), EwCase(5, 16383, 64, False), EwCase(5, 16386, 64, True)]

# gp_fwd: B, n, trips of the `i += 256` loop, waves with data
GpCase = namedtuple("GpCase", "B n trips waves_with_data")
GP_CASES = [GpCase(6, 150, 1, 3), GpCase(6, 255, 1, 4), GpCase(6, 256, 1, 4), GpCase(6, 257, 2, 4), GpCase(6, 3000, 12, 4),
            GpCase(6, 16386, 65, 4)]
# gp_bwd: the same shapes, and one whose blockIdx.y runs over a whole batch
GP_BWD_CASES = [EwCase(6, 150, 1, False), EwCase(6, 255, 1, False), EwCase(6, 256, 1, False), EwCase(6, 257, 2, False),
                EwCase(6, 3000, 12, False), EwCase(6, 16386, 64, True), EwCase(64, 150, 1, False)]

# wgan_losses: B, T, trips over B * T, waves with data, trips over pen [B]
WganCase = namedtuple("WganCase", "B T trips waves_with_data pen_trips")
WGAN_CASES = [WganCase(8, 3, 1, 1, 1), WganCase(64, 3, 1, 3, 1), WganCase(86, 3, 2, 4, 1), WganCase(300, 1, 2, 4, 2)]
WGAN_FORMS = ["real+pen", "real", "generator"]

# argmax_rows: rows, V, padding of the row stride (ld = V + pad), trips per lane, idle waves of the last workgroup
ArgmaxCase = namedtuple("ArgmaxCase", "rows V pad trips idle_waves")
ARGMAX_V = {50: 1, 64: 1, 65: 2, 1000: 16}                # V: trips (50: lanes 50 .. 63 read nothing; 64: one full trip)
ARGMAX_R = {1: 3, 5: 3, 24: 0, 193: 3}                     # rows: idle waves (193: in the 49th workgroup)
ARGMAX_CASES = [ArgmaxCase(rows, V, pad, trips, idle) for V, trips in ARGMAX_V.items() for rows, idle in ARGMAX_R.items()
                for pad in (0, 24)]

# spatial means: B, npass (R = B * npass), L, C; forward: row groups without a row, unequal rows per group, the `c < C` guard;
# backward: blockIdx.y slices, most rows per slice, unequal rows per slice
SmCase = namedtuple("SmCase", "B npass L C empty_groups ragged_groups c_guard gy y_trips ragged_y")
SM_CASES = [
    SmCase(3, 2, 16, 512, 0, False, False, 16, 1, False),
    SmCase(2, 1, 5, 512, 3, True, False, 5, 1, False),            # L < 8
    SmCase(2, 3, 196, 512, 0, True, False, 16, 13, True),         # the 14 x 14 feature map
    SmCase(1, 2, 784, 256, 0, False, False, 16, 49, False),       # the 28 x 28 one
    SmCase(2, 2, 12, 132, 0, True, True, 12, 1, False),           # gy = L; C no multiple of 128 (nor of 256)
]
