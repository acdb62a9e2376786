"""numpy fp64 restatement of the two entry points of csrc/relax.hip (definitions in include/sgg_hip.h, "relaxed generator output"):
Philox4x32-10, the mapping of its words to u in (0, 1), the relaxation y = softmax((x + g) / tau) and its gradient.  Shared by
tests/test_relax_cpu.py and tests/test_relax_gpu.py."""
import numpy as np

# Tolerances, device fp32 against this fp64 restatement: 10 x the largest error measured on the MI355X over the cases of
# tests/test_relax_gpu.py (RELAX_CASES x tau in {1.0, 0.25} x both modes x in place / out of place), rounded up - the project's
# margin everywhere (tests/tolerances.py).
#   forward: RELAX_ERR_MEASURED = the largest |y - y64|, y in [0, 1]: 5.88e-7 at R = 9, V = 64, tau 0.25 with Gumbel noise (the
#   fp32 g = -log(-log u) is up to an ulp of 16 off and tau 0.25 multiplies that by four before the exp; at tau 1 at most 3.2e-7, at
#   V = 70 001); without noise at most 3.33e-7 (V = 5125 and 70 001 at tau 0.25), 1.5e-7 at the workload's V = 1000.
#   backward: RELAX_GRAD_ERR_MEASURED = the largest |dx - dx64| in units of max|dy| * scale / tau (absolute in that unit, not
#   relative to max|dx|: a saturated row's gradients are differences of nearly equal numbers): 6.76e-8 at R = 1025, V = 7 (6.0e-8
#   at V = 65; from V = 1000 up at most 5.4e-8) - y and dy are the kernel's inputs, so only its dot product and three roundings count.
RELAX_ERR_MEASURED = 5.9e-7
RELAX_GRAD_ERR_MEASURED = 6.8e-8
RELAX_TOL = 6e-6
RELAX_GRAD_TOL = 7e-7

M32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85


def philox4x32(counter, key, rounds=10):
    """The Philox4x32 block function: counter = four uint64 arrays (or ints) holding 32-bit words, key = two -> four uint64 arrays."""
    c = [np.asarray(w, dtype=np.uint64) & np.uint64(M32) for w in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & M32, int(key[1]) & M32
    for _ in range(rounds):
        p0, p1 = np.uint64(PHILOX_M0) * c[0], np.uint64(PHILOX_M1) * c[2]             # (32 x 32 -> 64 bits: no overflow in uint64)
        h0, l0 = p0 >> np.uint64(32), p0 & np.uint64(M32)
        h1, l1 = p1 >> np.uint64(32), p1 & np.uint64(M32)
        c = [h1 ^ c[1] ^ np.uint64(k0), l1, h0 ^ c[3] ^ np.uint64(k1), l0]
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c


def u_of_word(w):
    """u = ((w >> 9) + 0.5) * 2^-23: 23 bits, exact in fp32, strictly inside (0, 1)."""
    return ((np.asarray(w, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def uniforms(seed, draw, R, V, row0=0):
    """u [R, V] fp64 of rows row0 .. row0 + R - 1: key (seed lo, seed hi), counter (j >> 2, r, draw lo, draw hi), word j & 3."""
    seed, draw = int(seed) & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1)
    j = np.arange(V, dtype=np.uint64)[None, :]
    r = np.arange(row0, row0 + R, dtype=np.uint64)[:, None]
    words = philox4x32((j >> np.uint64(2), r, draw & M32, draw >> 32), (seed & M32, seed >> 32))
    sel = (j & np.uint64(3)) + np.zeros_like(r)
    w = np.choose(sel.astype(np.int64), [np.broadcast_to(x, sel.shape) for x in words])
    return u_of_word(w)


def gumbel(u):
    return -np.log(-np.log(np.asarray(u, dtype=np.float64)))


def relax_rows(x, tau, gumbel_noise=False, seed=0, draw=0):
    """x [R, V] (as given: float32 on the GPU side) -> (y [R, V] fp64, u [R, V] fp64 or None)."""
    x = np.asarray(x, dtype=np.float64)
    u = uniforms(seed, draw, x.shape[0], x.shape[1]) if gumbel_noise else None
    z = (x + (gumbel(u) if gumbel_noise else 0.0)) / float(tau)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True), u


def relax_rows_bwd(y, dy, tau, scale=1.0):
    """dx_j = (scale / tau) * y_j * (dy_j - sum_k y_k dy_k), fp64."""
    y, dy = np.asarray(y, dtype=np.float64), np.asarray(dy, dtype=np.float64)
    return (float(scale) / float(tau)) * y * (dy - (y * dy).sum(axis=1, keepdims=True))
