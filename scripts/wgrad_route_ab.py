"""Filter gradients of one library against another's, bit for bit.

  python scripts/wgrad_route_ab.py --lib PATH --out FILE        run the case table on the library at PATH, write one line per case
  python scripts/wgrad_route_ab.py --compare FILE_A FILE_B      the two-column result; exit status 1 unless every digest is equal
                                        [--labels A B]          (what the two sides are called in the output; default: the paths)
  python scripts/wgrad_route_ab.py --traces CSV_A CSV_B FILE_B  the kernel traces of two such runs (rocprofv3 --kernel-trace
                                                                --output-format csv): per case the sequence of (kernel, grid) must be
                                                                equal, and equal to the symbols FILE_B recorded

The run binds the C entry points that every version of the library has (sgg_conv2d_nhwc_wgrad, _workspace_bytes, sgg_presplit16,
sgg_absmax, sgg_fill) directly with ctypes, so that it loads a library built from an older commit as well; where the library has
sgg_conv2d_nhwc_wgrad_symbol its answer is recorded beside the digest.  Cases: at least one per kernel family and template arm of the
filter gradient, at the smallest shapes that reach it.  A line: name, SHA-256 of dw, reported symbols ("-" if none).  Every case
starts with ONE sgg_fill launch (dw poisoned with NaN), which is how --traces cuts a trace into cases."""
import argparse
import ctypes
import csv
import hashlib
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, H, W, Cin, Cout, k, stride) of tests/test_presplit_gpu.py: WGRAD_BAND_CASES, DMA_CASES
BAND = [(2, 56, 56, 64, 128, 5, 2), (3, 28, 28, 128, 64, 5, 2), (1, 14, 14, 64, 64, 5, 2), (3, 20, 20, 64, 64, 3, 1), (1, 9, 9, 64, 128, 3, 1)]
DMA = [(2, 16, 16, 64, 128, 3, 1), (3, 24, 16, 128, 128, 3, 1), (2, 8, 8, 256, 256, 3, 1), (5, 40, 24, 64, 64, 3, 1), (1, 8, 16, 128, 64, 3, 1),
       (3, 32, 32, 128, 128, 5, 2), (2, 16, 48, 64, 128, 5, 2), (3, 56, 56, 64, 128, 5, 2), (2, 28, 28, 128, 64, 5, 2), (2, 20, 20, 64, 64, 3, 1),
       (1, 9, 9, 64, 128, 3, 1)]


def cases():
    """(shape, precision, algo, operand_format, ln)"""
    out = []
    for sh in BAND:                                     # halo row bands: f32 operands, one pre-split, single-piece modes
        out += [(sh, 2, 0, 0, 0), (sh, 2, 0, 1, 0), (sh, 3, 0, 0, 0), (sh, 1, 0, 0, 0), (sh, 4, 0, 0, 0)]
    out += [(sh, 2, 0, 3, 0) for sh in DMA]             # LDS-DMA: 64 x 128 and 64 x 64 tiles, parity classes, row bands
    for ci, co in ((32, 32), (32, 64), (64, 64)):       # halo 8x8 blocks: the three channel chunks
        sh = (2, 16, 16, ci, co, 3, 1)
        out += [(sh, 2, 0, 0, 0), (sh, 2, 0, 2, 0), (sh, 2, 0, 3 if ci == 32 else 1, 0), (sh, 3, 0, 0, 0), (sh, 1, 0, 0, 0), (sh, 4, 0, 0, 0),
                (sh, 2, 0, 0, 1), (sh, 3, 0, 0, 1)]
    sh = (2, 16, 16, 64, 128, 3, 1)
    out += [(sh, 1, 0, 0, 0), (sh, 2, 0, 0, 0), (sh, 3, 0, 0, 0), (sh, 2, 0, 0, 1), (sh, 3, 0, 0, 1), (sh, 2, 0, 2, 1)]
    for ci, co in ((32, 32), (32, 64), (64, 64)):       # 5x5 stride 2 on a 16 x 16 dy grid: the four parity classes on the halo kernel
        sh = (2, 32, 32, ci, co, 5, 2)
        out += [(sh, 2, 0, 0, 0), (sh, 3, 0, 0, 0), (sh, 2, 0, 0, 1), (sh, 3, 0, 0, 1), (sh, 1, 0, 0, 0), (sh, 4, 0, 0, 0)]
    out += [((2, 32, 32, 64, 128, 5, 2), 2, 0, 3, 0), ((2, 32, 32, 64, 64, 5, 2), 2, 0, 3, 0)]       # ... and by LDS-DMA
    sh = (2, 12, 12, 128, 128, 3, 1)                    # per-tap: 128 x 128 tiles, f32 and transposed
    out += [(sh, 0, 0, 0, 0), (sh, 6, 0, 0, 0), (sh, 2, 1, 0, 0), (sh, 3, 1, 0, 0), (sh, 0, 1, 0, 0)]
    tiles = ((32, 32), (32, 64), (64, 32), (64, 64), (32, 128), (128, 32), (64, 128), (128, 64))
    for ci, co in tiles:                                # per-tap: the other channel tiles, in f32, fp16 pieces, two and three bf16 pieces
        out += [((2, 12, 12, ci, co, 3, 1), precision, 1, 0, 0) for precision in (0, 2, 3, 6)]
    out += [((1, 12, 12, 64, 64, 3, 1), 2, 1, 0, 0),    # one pixel split: dw written directly
            ((2, 31, 31, 64, 64, 5, 2), 2, 0, 0, 0),    # odd x grid under stride 2: per-tap with stride and pads
            ((2, 16, 32, 3, 32, 3, 1), 2, 0, 0, 0), ((3, 9, 33, 3, 32, 3, 1), 0, 0, 0, 0)]       # Cin = 3
    return out


def same_pads(n, k, s):
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return out, total // 2


def run(lib_path, out_path):
    import torch
    L = ctypes.CDLL(lib_path)
    vp, i, ll, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_size_t
    L.sgg_last_error.restype = ctypes.c_char_p
    L.sgg_conv2d_nhwc_wgrad_workspace_bytes.restype, L.sgg_conv2d_nhwc_wgrad_workspace_bytes.argtypes = sz, [i] * 9
    L.sgg_conv2d_nhwc_wgrad.restype = i
    L.sgg_conv2d_nhwc_wgrad.argtypes = [vp, vp, vp] + [i] * 14 + [vp, vp, vp, vp, vp, i, vp, sz, vp]
    L.sgg_presplit16.restype, L.sgg_presplit16.argtypes = i, [vp, vp, ll, vp, vp]
    L.sgg_absmax.restype, L.sgg_absmax.argtypes = i, [vp, ll, vp, vp]
    L.sgg_fill.restype, L.sgg_fill.argtypes = i, [vp, ll, ctypes.c_float, vp]
    query = getattr(L, "sgg_conv2d_nhwc_wgrad_symbol", None)
    if query is not None:
        query.restype, query.argtypes = i, [i] * 16 + [vp, ctypes.c_char_p, i]

    def check(rc, what):
        if rc != 0:
            raise RuntimeError("%s: %d %s" % (what, rc, L.sgg_last_error().decode()))

    def rnd(shape, seed):
        return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)

    lines = []
    for n, ((B, H, W, Ci, Co, k, s), precision, algo, fmt, ln) in enumerate(cases()):
        (Ho, pt), (Wo, pl) = same_pads(H, k, s), same_pads(W, k, s)
        dims = (B, H, W, Ci, Ho, Wo, Co, k, k, s, pt, pl)
        name = "%dx%dx%dx%d->%d_k%ds%d_p%d_a%d_f%d_ln%d" % (B, H, W, Ci, Co, k, s, precision, algo, fmt, ln)
        xh, dyh = rnd((B, H, W, Ci), 5 + n), rnd((B, Ho, Wo, Co), 105 + n)
        x, dy = xh.cuda(), dyh.cuda()
        dw = torch.empty((k, k, Ci, Co), device="cuda")
        ws = torch.full((max(1, L.sgg_conv2d_nhwc_wgrad_workspace_bytes(*dims[:9])) // 4 + 1,), float("nan"), device="cuda")
        am = torch.zeros(2, device="cuda")
        lnp = [None, None, None]
        if ln:          # x is the producing layer's pre-LayerNorm output; the amax word bounds max|ELU(LN(x))|
            mean, var = xh.mean(dim=(1, 2, 3)), xh.var(dim=(1, 2, 3), unbiased=False)
            stats = torch.stack([mean, (var + 1e-12).rsqrt()], dim=1).contiguous()
            gamma, beta = 1.0 + 0.1 * rnd((Ci,), 300 + n), 0.1 * rnd((Ci,), 400 + n)
            a = torch.nn.functional.elu((xh - stats[:, 0].view(B, 1, 1, 1)) * stats[:, 1].view(B, 1, 1, 1) * gamma + beta)
            am[0] = 1.5 * float(a.abs().max())
            lnp = [stats.cuda(), gamma.cuda(), beta.cuda()]
        torch.cuda.synchronize()
        check(L.sgg_fill(dw.data_ptr(), dw.numel(), float("nan"), None), "sgg_fill")         # (the case marker of --traces)
        if not ln:
            check(L.sgg_absmax(x.data_ptr(), x.numel(), am.data_ptr(), None), "sgg_absmax")
        check(L.sgg_absmax(dy.data_ptr(), dy.numel(), am[1:].data_ptr(), None), "sgg_absmax")
        if fmt & 1:
            check(L.sgg_presplit16(x.data_ptr(), x.data_ptr(), x.numel(), am.data_ptr(), None), "sgg_presplit16")
        if fmt & 2:
            check(L.sgg_presplit16(dy.data_ptr(), dy.data_ptr(), dy.numel(), am[1:].data_ptr(), None), "sgg_presplit16")
        check(L.sgg_conv2d_nhwc_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), *dims, precision, algo, am.data_ptr(), am[1:].data_ptr(),
                                      *[None if t is None else t.data_ptr() for t in lnp], fmt, ws.data_ptr(), ws.numel() * 4, None), name)
        torch.cuda.synchronize()
        out = dw.cpu()
        if not bool(torch.isfinite(out).all()):
            raise RuntimeError("%s: dw is not finite" % name)
        syms = "-"
        if query is not None:
            buf = ctypes.create_string_buffer(256)
            check(query(*dims, precision, algo, ln, fmt, None, buf, len(buf)), "sgg_conv2d_nhwc_wgrad_symbol")
            syms = buf.value.decode()
        lines.append("%s %s %s" % (name, hashlib.sha256(out.numpy().tobytes()).hexdigest(), syms))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("%d cases -> %s" % (len(lines), out_path))


def read(path):
    return [line.split() for line in open(path) if line.strip()]


def compare(path_a, path_b, labels):
    a, b = read(path_a), read(path_b)
    same = len(a) == len(b)
    print("# SHA-256 of dw per case: %s | %s" % tuple(labels or (path_a, path_b)))
    for ra, rb in zip(a, b):
        ok = ra[:2] == rb[:2]
        same &= ok
        print("%-44s %s %s %s" % (ra[0], ra[1][:20], rb[1][:20], "equal" if ok else "DIFFERENT (%s)" % rb[0]))
    print("RESULT: %d cases, %s" % (len(a), "every digest equal" if same else "DIGESTS DIFFER"))
    return 0 if same else 1


def trace_cases(path):
    """Per case (cut at the fill kernel) the (name, grid) of the filter-gradient kernels and the slab reduce, in start order."""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r.get("Dispatch_Id") or r["Start_Timestamp"]))
    pat = re.compile(r"^(?:void)?((?:conv_wgrad|conv_c3_wgrad|slab_reduce)\w*(?:<[^>]*>)?)")
    out = []
    for r in rows:
        name = r["Kernel_Name"].replace(" ", "")
        if re.match(r"^(?:void)?fill4?_kernel", name):       # sgg_fill: one launch (dw has a multiple of four elements)
            out.append([])
        m = pat.match(name)
        if m and out:
            out[-1].append((m.group(1), "x".join(r[key] for key in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z") if key in r) or r.get("Grid_Size", "?")))
    return out


def traces(csv_a, csv_b, file_b, labels):
    ta, tb, rec = trace_cases(csv_a), trace_cases(csv_b), read(file_b)
    same = len(ta) == len(tb) == len(rec)
    print("# rocprofv3 --kernel-trace of two runs of this script: kernels and grids (work-items) per case; A = %s, B = %s" % tuple(labels or (csv_a, csv_b)))
    for a, b, (name, _, syms) in zip(ta, tb, rec):
        conv = ";".join(k for k, _ in b if not k.startswith("slab_reduce"))
        ok, rep = a == b, conv == syms
        same &= ok and rep
        print("%s: %s | A %s B, reported %s the trace" % (name, " ".join("%s[%s]" % kg for kg in b), "==" if ok else "!=", "==" if rep else "!="))
        if not ok:
            print("    A: %s" % " ".join("%s[%s]" % kg for kg in a))
        if not rep:
            print("    reported: %s" % syms)
    print("RESULT: %d cases, %s" % (len(rec), "sequences equal, and equal to the reported symbols" if same else "SEQUENCES DIFFER"))
    return 0 if same else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--traces", nargs=3)
    ap.add_argument("--labels", nargs=2)
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare, args.labels))
    if args.traces:
        sys.exit(traces(*args.traces, args.labels))
    run(args.lib, args.out)
