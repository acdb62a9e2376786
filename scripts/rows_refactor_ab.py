"""rows_refactor_ab.py - the row kernels (csrc/xent.hip, csrc/relax.hip, argmax_rows) of one library against another's, in one process:
bits, then time.

    python scripts/rows_refactor_ab.py --parent PATH [--new PATH] [--repeats 20] [--out FILE]

Both libraries are loaded with ctypes (--new defaults to the tree's own libsgg_hip.so); diff_bits, the library wrapper and the
alternating burst timing are those of scripts/optim_refactor_ab.py.

  bits    sgg_softmax_xent on XENT_CASES (tests/test_xent_gpu.py: all outputs with accumulate 0 and 1, and the lse-only mode);
          sgg_relax_rows, sgg_relax_rows_bwd, sgg_relax_rows_hard, sgg_relax_rows_hard_bwd and sgg_argmax_rows on RELAX_CASES
          (tests/test_relax_gpu.py) and on DX_APART_CASE (both inputs aligned alike, dx one element off: the vectorised pass 1 with the
          scalar pass 2): softmax and Gumbel, tau 1.0 and 0.25, u_out and tok present and absent, y alone, out of place and in place
          (y on x, dx on dy).  Inputs and the layouts of the rows are the tests'; the WHOLE buffer around every output is compared, the
          guard words between and behind the rows included.  Reported: the number of differing BITS per output, summed over the
          cases.  Required: zero everywhere.
  timing  R = 192 rows at V = 1000 (resident) and V = 70 000 (streaming): xent with gradient, soft forward with Gumbel, soft backward,
          hard forward with Gumbel, hard backward with Gumbel; argmax at V = 1000.  Bursts between two device events, parent and new
          alternating, --repeats repetitions.  Required: the median of the new library does not exceed the parent's slowest
          repetition of the same leg (the parent's own spread in the same run is the noise).

Prints ONE JSON line (with --out also into FILE); exit status 1 unless both requirements hold.  Needs the GPU; reads nothing outside the
repository except the two libraries."""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import optim_refactor_ab as AB  # noqa: E402

TAUS = (1.0, 0.25)
SCALE = 0.37
TIMING_R, TIMING_V = 192, (1000, 70000)


class Lib(AB.Lib):
    def __init__(self, path):
        L = self.L = ctypes.CDLL(path)
        vp, i, ll, ull, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_float
        L.sgg_last_error.restype = ctypes.c_char_p
        for name, args in (("sgg_softmax_xent", [vp, ll, i, i, vp, f, i, vp, ll, vp, vp, vp, vp]),
                           ("sgg_relax_rows", [vp, ll, i, i, f, i, ull, ull, vp, ll, vp, ll, vp]),
                           ("sgg_relax_rows_bwd", [vp, ll, vp, ll, i, i, f, f, vp, ll, vp]),
                           ("sgg_relax_rows_hard", [vp, ll, i, i, i, ull, ull, vp, ll, vp, vp]),
                           ("sgg_relax_rows_hard_bwd", [vp, ll, vp, ll, i, i, f, f, i, ull, ull, vp, ll, vp]),
                           ("sgg_argmax_rows", [vp, vp, i, i, i, vp])):
            getattr(L, name).restype, getattr(L, name).argtypes = i, args


def bits_leg(libs):
    from tests.test_relax_cpu import SEED
    from tests.test_relax_gpu import DX_APART_CASE, DX_APART_SHIFT, RELAX_CASES, on_device, relax_case
    from tests.test_xent_gpu import F32, I32, SENT, XENT_CASES, rows_view, vec, xent_case
    out, cases = {}, 0

    def run(what, fn):
        """fn(lib) -> {name: buffer} on fresh buffers per library; the buffers are compared."""
        nonlocal cases
        res = []
        for lib in libs:
            res.append(fn(lib))
            torch.cuda.synchronize()
        for k in res[0]:
            out["%s.%s" % (what, k)] = out.get("%s.%s" % (what, k), 0) + AB.diff_bits(res[0][k], res[1][k])
        cases += 1

    for case in XENT_CASES:
        R, V, ld, ldd, sx, sd = case
        x, lab, _ = xent_case(case)
        labels = torch.from_numpy(lab).cuda()
        bx, xv = on_device(x, R, V, ld, sx, float("nan"))
        for acc in (0, 1):
            def xent(lib):
                bd, dv = rows_view(R, V, ldd, sd, SENT[F32])
                dv.fill_(0.125)
                (bn, nll), (bl, lse), (bh, hit) = vec(R, F32), vec(R, F32), vec(R, I32)
                lib.call("sgg_softmax_xent", xv, ld, R, V, labels, SCALE, acc, dv, ldd, nll, lse, hit)
                return {"dlogits": bd, "nll": bn, "lse": bl, "hit": bh, "logits": bx}
            run("softmax_xent[accumulate %d]" % acc, xent)

        def lse_only(lib):
            bl, lse = vec(R, F32)
            lib.call("sgg_softmax_xent", xv, ld, R, V, None, 1.0, 0, None, 0, None, lse, None)
            return {"lse": bl}
        run("softmax_xent[lse only]", lse_only)

    for case in list(RELAX_CASES) + [DX_APART_CASE]:
        R, V, ldx, ldy, sx, sy = case
        x, dy = relax_case(case, 1.0, False)[:2]
        draw = 77 + R
        # (rows, shift) of the backward operands: the tests' layouts; the added case keeps both inputs alike and moves dx alone
        apart = DX_APART_SHIFT if case == DX_APART_CASE else 0
        soft_l = ((ldy, sy), (ldx, sx), (ldy, sy + apart))          # y, dy, dx
        hard_l = ((ldx, sx), (ldy, sy), (ldx, sx + apart))          # x, dy, dx
        bx, xv = on_device(x, R, V, ldx, sx, float("nan"))
        def argmax(lib):
            am = torch.full((R,), -5, dtype=torch.int64, device="cuda")
            lib.call("sgg_argmax_rows", xv, am, R, V, ldx)
            return {"out": am}
        run("argmax_rows", argmax)
        for gumbel in (0, 1):
            def hard(lib, with_y, with_tok, in_place):
                bi, xi = on_device(x, R, V, ldx, sx, SENT[F32]) if in_place else (bx, xv)
                by, yv = (bi, xi) if in_place else on_device(None, R, V, ldy, sy, SENT[F32])
                tok = torch.full((R,), -5, dtype=torch.int64, device="cuda")
                lib.call("sgg_relax_rows_hard", xi, ldx, R, V, gumbel, SEED, draw, yv if with_y else None, ldx if in_place else ldy,
                         tok if with_tok else None)
                return {"y": by, "tok": tok}
            for tag, args in (("y+tok", (True, True, False)), ("y", (True, False, False)), ("tok", (False, True, False)),
                              ("in place", (True, True, True))):
                run("relax_rows_hard[%s]" % tag, lambda lib: hard(lib, *args))
            for tau in TAUS:
                def soft(lib, with_u, in_place):
                    bi, xi = on_device(x, R, V, ldx, sx, SENT[F32]) if in_place else (bx, xv)
                    by, yv = (bi, xi) if in_place else on_device(None, R, V, ldy, sy, SENT[F32])
                    bu, uv = on_device(None, R, V, ldy, sy, SENT[F32])
                    lib.call("sgg_relax_rows", xi, ldx, R, V, tau, gumbel, SEED, draw, yv, ldx if in_place else ldy,
                             uv if with_u else None, ldy if with_u else 0)
                    return {"y": by, "u_out": bu}
                run("relax_rows[u_out]" if gumbel else "relax_rows", lambda lib: soft(lib, bool(gumbel), False))
                run("relax_rows[in place]", lambda lib: soft(lib, False, True))
                # the backwards' y: the parent's soft row, the same input for both libraries
                ys = torch.empty(R, V, device="cuda")
                libs[0].call("sgg_relax_rows", xv, ldx, R, V, tau, gumbel, SEED, draw, ys, V, None, 0)

                def bwd(lib, name, a, layouts, on_dy, extra):
                    (lda, sa), (ldg, sg), (ldd, sd) = layouts
                    ba, av = on_device(a, R, V, lda, sa, float("nan"))
                    bg, gv = on_device(dy, R, V, ldg, sg, SENT[F32])
                    bd, dv = (bg, gv) if on_dy else on_device(None, R, V, ldd, sd, SENT[F32])
                    lib.call(name, av, lda, gv, ldg, R, V, tau, SCALE, *extra, dv, ldg if on_dy else ldd)
                    return {"dx": bd, "dy": bg}
                for on_dy in (False, True):
                    tag = "[dx on dy]" if on_dy else ""
                    run("relax_rows_bwd" + tag, lambda lib: bwd(lib, "sgg_relax_rows_bwd", ys.cpu().numpy(), soft_l, on_dy, ()))
                    run("relax_rows_hard_bwd" + tag, lambda lib: bwd(lib, "sgg_relax_rows_hard_bwd", x, hard_l, on_dy, (gumbel, SEED, draw)))
    return {"xent_cases": len(XENT_CASES), "relax_cases": len(RELAX_CASES) + 1, "taus": list(TAUS), "launch_pairs": cases,
            "differing_bits": out, "ok": not any(out.values())}


def timing_leg(libs, names, repeats, burst=10):
    R = TIMING_R
    gen = torch.Generator(device="cuda").manual_seed(11)
    fns, legs = [{} for _ in libs], []
    for V in TIMING_V:
        x = 4.0 * torch.randn(R, V, generator=gen, device="cuda")
        dy = torch.randn(R, V, generator=gen, device="cuda")
        lab = torch.randint(0, V, (R,), generator=gen, device="cuda")
        y, d = torch.empty_like(x), torch.empty_like(x)
        nll, lse = torch.empty(R, device="cuda"), torch.empty(R, device="cuda")
        hit, tok = torch.empty(R, dtype=torch.int32, device="cuda"), torch.empty(R, dtype=torch.int64, device="cuda")
        libs[0].call("sgg_relax_rows", x, V, R, V, 0.5, 1, 3, 4, y, V, None, 0)
        ys = y.clone()
        for lib, f in zip(libs, fns):
            def add(leg, fn):
                f["%s/V%d" % (leg, V)] = fn
            add("xent_grad", lambda lib=lib, x=x, lab=lab, d=d, V=V, nll=nll, lse=lse, hit=hit:
                lib.call("sgg_softmax_xent", x, V, R, V, lab, 1.0, 0, d, V, nll, lse, hit))
            add("relax_rows_gumbel", lambda lib=lib, x=x, y=y, V=V: lib.call("sgg_relax_rows", x, V, R, V, 0.5, 1, 3, 4, y, V, None, 0))
            add("relax_rows_bwd", lambda lib=lib, ys=ys, dy=dy, d=d, V=V: lib.call("sgg_relax_rows_bwd", ys, V, dy, V, R, V, 0.5, 1.0, d, V))
            add("relax_rows_hard_gumbel", lambda lib=lib, x=x, y=y, tok=tok, V=V: lib.call("sgg_relax_rows_hard", x, V, R, V, 1, 3, 4, y, V, tok))
            add("relax_rows_hard_bwd_gumbel", lambda lib=lib, x=x, dy=dy, d=d, V=V:
                lib.call("sgg_relax_rows_hard_bwd", x, V, dy, V, R, V, 0.5, 1.0, 1, 3, 4, d, V))
            if V == TIMING_V[0]:
                add("argmax_rows", lambda lib=lib, x=x, tok=tok, V=V: lib.call("sgg_argmax_rows", x, tok, R, V, V))
    legs = list(fns[0])
    res = {"rows": R, "burst": burst, "repeats": repeats, "order": "%s first in even repetitions, %s first in odd ones" % tuple(names),
           "legs": AB.alternating_bursts(fns, legs, names, repeats, burst)}
    res["ok"] = all(v["new_median_within_parent_max"] for v in res["legs"].values())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--new", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import sgg_amd  # noqa: F401
    from sgg_amd.build import LIB_PATH
    libs = [Lib(args.parent), Lib(args.new or LIB_PATH)]
    rec = {"metric": "rows_refactor_ab", "parent": os.path.basename(args.parent), "new": os.path.basename(args.new or LIB_PATH),
           "bits": bits_leg(libs), "timing": timing_leg(libs, ("parent", "new"), args.repeats), "device": torch.cuda.get_device_name(0)}
    rec["ok"] = rec["bits"]["ok"] and rec["timing"]["ok"]
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0 if rec["ok"] else 1)


if __name__ == "__main__":
    main()
