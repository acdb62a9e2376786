"""Writes tests/golden/head_symbols.json: the kernels of the head GEMM and attention launches over a grid of their scalars, from a
Python restatement of the three dispatch ladders of csrc/gemm.hip (gemm_plan, gemm_wk_applicable, gemm_wk_tm, gemm_run) and
csrc/head.hip (sgg_attn_step_fwd, sgg_attn_step_bwd) as they stood before the library reported its routes itself
(sgg_gemm_skinny_symbol, sgg_attn_step_fwd_symbol, sgg_attn_step_bwd_symbol).  tests/test_head_routes_cpu.py holds the library to
the table.  One deliberate difference from that dispatch: the fused float backward is refused beyond 150 KB of LDS like the
dual one (the launch itself used to fail there).  With --check this script compares the restatement with the library row by row instead of writing.

    python scripts/head_route_table.py [--check]
"""
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "head_symbols.json")

SGG_LDK, ATTN_ROWS_CS, ATTN_MAX_PASS = 36, 128, 4        # csrc/mma_f32.h, csrc/head.hip


def cdiv(a, b):
    return (a + b - 1) // b


# ---- csrc/gemm.hip ----------------------------------------------------------------------------------------------------------
def gemm_plan(M, N, K):
    tiles = cdiv(M, 64) * cdiv(N, 64)
    ns = 1
    if tiles < 256 and K >= 2048:
        ns = max(min(cdiv(512, tiles), max(K // 512, 1)), 1)
    elif tiles < 128 and K >= 512:
        ns = max(min(cdiv(256, tiles), K // 64), 1)
    elif tiles < 64 and K >= 128:
        ns = max(min(K // 64, 64 // tiles), 1)
    kc = max(cdiv(cdiv(K, ns), 32) * 32, 32)
    return max(cdiv(K, kc), 1), kc


def gemm_wk_tm(M, N):
    ntn = cdiv(N, 16)
    for c in (6, 4, 2, 1):
        if c * 16 <= cdiv(M, 16) * 16 and cdiv(M, 16 * c) * ntn >= 224:
            return c
    return 1


def gemm_wk_applicable(mode, M, N, K, nsplit):
    if 64 < M <= 128 and N * K >= 1 << 21:
        return False
    return mode != 2 and nsplit > 1 and M <= 512 and K <= 8192 and N >= 16


def gemm_symbol(mode, M, N, K):
    """(kernels, nsplit) or ("refused: <text>", 0)."""
    if not (M > 0 and N > 0 and K > 0):
        return "refused: M, N, K must be positive", 0
    ns, _ = gemm_plan(M, N, K)
    tb = "true" if mode == 1 else "false"
    if gemm_wk_applicable(mode, M, N, K, ns):
        tm = gemm_wk_tm(M, N)
        return "gemm_wk_kernel<%d,%s,%d>" % (tm, tb, 2 if tm >= 4 else 4), 1
    sym = "gemm_kernel<%s,%s>" % ("true" if mode == 2 else "false", tb)
    if ns > 1:
        sym += ";gemm_slab_reduce_wide_kernel" if ns >= 16 else ";gemm_slab_reduce_kernel"
    return sym, ns


# ---- csrc/head.hip ----------------------------------------------------------------------------------------------------------
def attn_check(R, B, L, C):
    if not (R > 0 and B > 0 and L > 0 and C > 0 and R % B == 0):
        return "refused: need R % B == 0"
    if C % 256:
        return "refused: C must be a multiple of 256"
    return None


def attn_rows_lds_bytes(tr, L):
    return (cdiv(L, 32) * tr * SGG_LDK + 2 * 32 * ATTN_ROWS_CS) * 4


def attn_fwd_symbol(R, B, L, C, dual):
    bad = attn_check(R, B, L, C)
    if bad:
        return bad
    N = R // B
    tr = 64 if attn_rows_lds_bytes(64, L) <= 112 * 1024 else 32
    if not dual and N >= 32 and attn_rows_lds_bytes(tr, L) <= 160 * 1024:
        return "attn_step_fwd_rows_kernel<%d>" % tr
    return "attn_step_fwd_kernel<%s>" % ("Dual" if dual else "float")


def attn_bwd_symbol(R, B, L, C, dual):
    bad = attn_check(R, B, L, C)
    if bad:
        return bad
    npass = R // B
    if npass > ATTN_MAX_PASS:
        return "refused: at most 4 rows per image"
    t = "Dual" if dual else "float"
    ls = min(512 // B, L // 8) if (B < 256 and 64 <= L <= 2048) else 1
    if ls > 1:
        return "attn_step_bwd_ctx_kernel<%s>;attn_step_bwd_softmax_kernel<%s>" % (t, t)
    if npass * (C + 2 * L) * (8 if dual else 4) > 150 * 1024:      # (the float launch had no such check: see the module docstring)
        return "refused: L too large for LDS"
    return "attn_step_bwd_kernel<%s>" % t


# ---- the grids --------------------------------------------------------------------------------------------------------------
def gemm_rows():
    from tests import head_shapes as HS
    import bench
    # both sides of every threshold: tiles = 63 | 64, 127 | 128, 255 | 256 through M and N; K = 127 | 128, 511 | 512, 2047 | 2048,
    # 8192 | 8193; M = 64 | 65, 128 | 129, 512 | 513; N = 15 | 16; N * K = 2^21 -+ ; the candidates of gemm_wk_tm through M and N
    Ms = [1, 16, 17, 49, 64, 65, 80, 81, 128, 129, 192, 512, 513, 1024]
    Ns = [1, 15, 16, 196, 300, 960, 1000, 1324, 2045, 2048, 4032, 4096]
    Ks = [1, 127, 128, 130, 511, 512, 1023, 1024, 1324, 2047, 2048, 8192, 8193, 70000]
    rows = set(itertools.product((0, 1, 2), Ms, Ns, Ks))
    for B, S, V in [bench.CONFIGS[i] for i in (1, 3, 4)] + [(128, 224, 1000), (8, 64, 50)]:
        for launch in HS.all_launches(B, HS.feature_locations(S), V):
            if launch[0] == "gemm":
                rows.add(launch[1:])
    rows |= {(0, 0, 16, 16), (1, 16, -1, 16), (2, 16, 16, 0)}
    return sorted(rows)


def attn_rows():
    # N = R / B = 31 | 32 (rows kernel), its LDS limits (64-row tiles up to L = 256, 32-row tiles up to L = 896), R = 255 | 256,
    # C % 512, L = 63 | 64, L = 2048 | 2049, B = 255 | 256, npass = 4 | 5, the LDS limit of the fused backward (9000 | 9600 dual)
    Bs = [1, 2, 64, 85, 128, 255, 256]
    Ns = [1, 2, 3, 31, 32]
    Ls = [16, 63, 64, 196, 256, 257, 896, 897, 2048, 2049, 9000, 9600]
    Cs = [256, 512, 384]
    fwd = [(B * N, B, L, C, d) for B, N, L, C, d in itertools.product(Bs, Ns, Ls, Cs, (0, 1))]
    bwd = [(B * N, B, L, C, d) for B, N, L, C, d in itertools.product(Bs, [1, 2, 4, 5], Ls, Cs, (0, 1))]
    extra = [(7, 2, 16, 512, 0), (0, 2, 16, 512, 0), (255, 255, 16, 512, 0), (255, 85, 16, 512, 0), (256, 128, 16, 512, 0)]
    return sorted(set(fwd + extra)), sorted(set(bwd + extra))


def table():
    """Rows grouped to keep the file small: GEMM rows [N, K, nsplit, symbol_index] under [mode, M]; attention rows
    [R, L, symbol_index] under [B, C, dual]."""
    symbols, index = [], {}

    def idx(s):
        if s not in index:
            index[s] = len(symbols)
            symbols.append(s)
        return index[s]

    def grouped(rows, key, rest):
        groups = []
        for k, members in itertools.groupby(sorted(rows, key=key), key=key):
            groups.append(list(k) + [[rest(r) for r in members]])
        return groups
    gemm = grouped(gemm_rows(), lambda r: (r[0], r[1]), lambda r: [r[2], r[3], gemm_symbol(*r)[1], idx(gemm_symbol(*r)[0])])
    fwd_rows, bwd_rows = attn_rows()
    key = lambda r: (r[1], r[3], r[4])
    fwd = grouped(fwd_rows, key, lambda r: [r[0], r[2], idx(attn_fwd_symbol(*r))])
    bwd = grouped(bwd_rows, key, lambda r: [r[0], r[2], idx(attn_bwd_symbol(*r))])
    return {"gemm_group_fields": ["mode", "M"], "gemm_row_fields": ["N", "K", "nsplit", "symbol_index"],
            "attn_group_fields": ["B", "C", "dual"], "attn_row_fields": ["R", "L", "symbol_index"],
            "symbols": symbols, "gemm": gemm, "attn_fwd": fwd, "attn_bwd": bwd}


def count(groups):
    return sum(len(g[-1]) for g in groups)


def main():
    t = table()
    sizes = tuple(count(t[k]) for k in ("gemm", "attn_fwd", "attn_bwd"))
    if "--check" in sys.argv:
        from tests.test_head_routes_cpu import library_differences
        wrong = library_differences(t)
        print("%d gemm, %d + %d attention rows, %d differ" % (sizes + (len(wrong),)))
        for w in wrong[:20]:
            print(w)
        return 1 if wrong else 0
    with open(GOLDEN, "w") as f:
        f.write("{\n")
        keys = list(t)
        for k in keys:
            v = t[k]
            if k in ("gemm", "attn_fwd", "attn_bwd"):
                body = "[\n" + ",\n".join("    " + json.dumps(g, separators=(",", ":")) for g in v) + "\n  ]"
            else:
                body = json.dumps(v)
            f.write('  %s: %s%s\n' % (json.dumps(k), body, "," if k != keys[-1] else ""))
        f.write("}\n")
    print("wrote %s: %d gemm, %d + %d attention rows, %d symbols" % ((GOLDEN,) + sizes + (len(t["symbols"]),)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
