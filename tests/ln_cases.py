"""How the streaming LayerNorm kernels cut a tensor into workgroups: a Python restatement of ln_geom (csrc/layernorm.hip), and the
cases of tests/test_layernorm_geometry_gpu.py (test infrastructure, importable without a GPU).

Every kernel of csrc/layernorm.hip takes its launch geometry from (B, HW * C) alone:

    nchunks = ceil(HW * C / LN_CHUNK)
    G   = min(ceil(SGG_LN_WGS / B), nchunks)      workgroups per sample
    cpg = ceil(nchunks / G)                       chunks each workgroup walks
    G   = ceil(nchunks / cpg)

At the batch-64 step conv1's LayerNorm (224 x 224 x 32) runs with G = 24 and cpg = 17; at the batches the other kernel tests use
(1 .. 4) cpg is 1 almost everywhere: the chunk loops make one trip, the running Chan merge of ln_stats_partial_kernel never merges,
and the sample loops of the parameter-gradient finalize make at most one trip per lane.  The cases below reach the batch-64 code
paths with planes of about 100 k elements per sample.  A change of SGG_LN_WGS or LN_CHUNK needs the same change here;
tests/test_ln_cases_cpu.py then says which case left the path it was built for.
"""
from collections import namedtuple

LN_WGS = 1536          # SGG_LN_WGS
LN_CHUNK = 4096        # LN_CHUNK
TS = 4                 # SGG_TS (csrc/sgg_common.h): floats per forward partial (count, mean, M2, max deviation)
LNF_BL = 32            # sample lanes of ln_bwd_finalize_body


def cdiv(a, b):
    return -(-a // b)


# nchunks: chunks per sample; G: workgroups per sample; cpg: chunks per workgroup; last: chunks the last workgroup walks;
# tail: N % LN_CHUNK (0: the last chunk is full)
Geometry = namedtuple("Geometry", "nchunks G cpg last tail")


def ln_geometry(B, HW, C):
    N = HW * C
    nchunks = cdiv(N, LN_CHUNK)
    G = max(1, min(cdiv(LN_WGS, B), nchunks))
    cpg = cdiv(nchunks, G)
    G = cdiv(nchunks, cpg)
    return Geometry(nchunks, G, cpg, nchunks - (G - 1) * cpg, N % LN_CHUNK)


def ln_workspace_bytes(B, HW, C):
    """sgg_layernorm_hwc_elu_workspace_bytes: part [B][G][TS], then sspart [B][G][2] and chpart [B][G][3][C], + 256."""
    G = ln_geometry(B, HW, C).G
    return B * G * (TS + 2 + 3 * C) * 4 + 256


def chunk_census(shape, region):
    """Per workgroup of one sample: the numbers of valid elements of the chunks it walks (a chunk past the end of the plane is not
    walked).  region None: every element is valid."""
    B, H, W, C = shape
    geo = ln_geometry(B, H * W, C)
    N = H * W * C
    out = []
    for g in range(geo.G):
        row = []
        for c in range(geo.cpg):
            base = (g * geo.cpg + c) * LN_CHUNK
            if base >= N:
                break
            end = min(N, base + LN_CHUNK)
            if region is None:
                row.append(end - base)
                continue
            y0, x0, hv, wv = region
            n = 0
            for pix in range(base // C, cdiv(end, C)):      # (C divides LN_CHUNK: a chunk holds whole pixels)
                py, px = divmod(pix, W)
                if y0 <= py < y0 + hv and x0 <= px < x0 + wv:
                    n += C
            row.append(n)
        out.append(row)
    return out


# id, shape (B, H, W, C), window (y0, x0, Hv, Wv) or None, G, cpg
Case = namedtuple("Case", "id shape region G cpg")

CASES = [
    # 25 chunks, the last one ragged (3072 of 4096), the last workgroup walks 1 chunk; B = 64: two finalize trips per sample lane
    Case("b64_c256", (64, 18, 22, 256), None, 13, 2),
    # B no multiple of 32: unequal trips; 23 chunks, ragged 3200; the C = 32 conv1 layer, also used for the fused conv1_1 gradient
    Case("b70_c32", (70, 54, 54, 32), None, 12, 2),
    # cpg = 4, the last workgroup walks 2 chunks, the last chunk ragged (3584); eight finalize trips per lane
    Case("b256_c128", (256, 25, 28, 128), None, 6, 4),
    # a canvas row is 2 chunks = one workgroup; rows 0, 1 and 15 lie outside the window: workgroups 0, 1 and 15 publish empty
    # partials through the early `continue`; columns 0 and 15 make every other chunk partly valid
    Case("b96_c512_win", (96, 16, 16, 512), (2, 1, 13, 14), 16, 2),
    # the odd-size canvas as the trunk plans it (window at the origin)
    Case("b96_c512_win0", (96, 16, 16, 512), (0, 0, 15, 15), 16, 2),
    # a canvas row is 1 chunk, a workgroup walks 2 rows: workgroup 0 is empty, workgroup 1 skips its first chunk and merges its second
    # into an EMPTY running partial (n_run = 0), workgroup 15 skips its second chunk after a valid first one
    Case("b96_c256_win_skip", (96, 32, 16, 256), (3, 1, 28, 14), 16, 2),
]
BY_ID = {c.id: c for c in CASES}
FUSED_C3_CASE = "b70_c32"      # conv1's LayerNorm: sgg_layernorm_hwc_elu_bwd_sums + sgg_conv2d_nhwc_wgrad_c3_ln
