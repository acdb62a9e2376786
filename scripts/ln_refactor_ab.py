"""ln_refactor_ab.py - the LayerNorm kernels (csrc/layernorm.hip) and the two conv1_1 kernels that compute the LayerNorm backward's dy
themselves, of one library against another's, in one process: bits, then time.

    python scripts/ln_refactor_ab.py --parent PATH [--new PATH] [--repeats 20] [--out FILE]

Both libraries are loaded with ctypes (--new defaults to the tree's own libsgg_hip.so); diff_bits, the library wrapper and the
alternating burst timing are those of scripts/optim_refactor_ab.py.

  bits    per problem (shape, valid window, inputs) every entry point on the same inputs, whole buffers compared - outputs, stats, the
          amax and pq words, means, and the whole workspace, zeroed before each call:
            sgg_layernorm_hwc_elu_fwd        f32 and pre-split, each with its own statistics pass and with tile_stats (the partials the
                                             statistics pass of the same library left in the workspace; whole planes only)
            sgg_layernorm_hwc_finalize       on the same partials
            sgg_layernorm_hwc_elu_bwd        f32 and pre-split, each with immediate and with deferred finalize, the deferred ones
                                             followed by sgg_layernorm_hwc_bwd_finalize
            sgg_presplit16                   of the f32 forward output under its maximum
            sgg_layernorm_hwc_elu_bwd_sums, sgg_conv2d_nhwc_wgrad_c3_ln, sgg_conv2d_nhwc_dgrad_c3_ln      (whole planes; the last two at C = 32)
          Problems: the six cases of tests/ln_cases.py with the inputs of tests/test_layernorm_geometry_gpu.py; the shapes and inputs of
          test_layernorm_elu and test_layernorm_elu_valid_region (tests/test_kernels_gpu.py) and of
          test_layernorm_outputs_presplit_are_todays_split_bit_for_bit (tests/test_presplit_gpu.py); the (2, 6, 8, 32) problem of
          test_layernorm_forward_presplit_from_the_convolutions_tile_partials with its host-made partials.
          Reported: the number of differing BITS per output, summed over the problems.  Required: zero everywhere.
  timing  B = 64 at the encoder's shapes for 224 px and one masked leg (112 x 112 x 64 canvas, window (0, 0, 111, 111)): forward f32
          with its own statistics pass, forward pre-split from tile_stats (the masked leg: from its own pass - tile_stats cover whole
          planes only), sgg_layernorm_hwc_finalize alone, backward f32 and pre-split with deferred finalize; bwd_sums +
          conv_c3_wgrad_ln and dgrad_c3_ln at 224 x 224 x 32.  Bursts between two device events, parent and new alternating, --repeats
          repetitions.  Required: the median of the new library does not exceed the parent's slowest repetition of the same leg (the
          parent's own spread in the same run is the noise).

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

TIMING_B = 64
TIMING_SHAPES = ((224, 224, 32), (112, 112, 64), (112, 112, 128), (56, 56, 256), (28, 28, 512))
TIMING_MASKED = ((112, 112, 64), (0, 0, 111, 111))


class Lib(AB.Lib):
    def __init__(self, path):
        L = self.L = ctypes.CDLL(path)
        vp, i, ll, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_size_t
        L.sgg_last_error.restype = ctypes.c_char_p
        for name, args in (("sgg_layernorm_hwc_elu_fwd", [vp] * 7 + [i] * 10 + [vp, sz, vp]),
                           ("sgg_layernorm_hwc_elu_bwd", [vp] * 10 + [i] * 9 + [vp, vp, sz, vp]),
                           ("sgg_layernorm_hwc_elu_bwd_sums", [vp] * 9 + [i] * 3 + [vp, sz, vp]),
                           ("sgg_layernorm_hwc_bwd_finalize", [vp, i, vp]),
                           ("sgg_layernorm_hwc_finalize", [vp, i] + [vp] * 4 + [i] * 3 + [vp]),
                           ("sgg_presplit16", [vp, vp, ll, vp, vp]),
                           ("sgg_conv2d_nhwc_wgrad_c3_ln", [vp] * 8 + [i] * 5 + [vp, sz, vp]),
                           ("sgg_conv2d_nhwc_dgrad_c3_ln", [vp] * 8 + [i] * 5 + [vp])):
            getattr(L, name).restype, getattr(L, name).argtypes = i, args
        L.sgg_layernorm_hwc_elu_workspace_bytes.restype, L.sgg_layernorm_hwc_elu_workspace_bytes.argtypes = sz, [i] * 3
        L.sgg_conv2d_nhwc_wgrad_workspace_bytes.restype, L.sgg_conv2d_nhwc_wgrad_workspace_bytes.argtypes = sz, [i] * 9


def region_args(region, W):
    return (0, 0, 0, 0, 0) if region is None else (W,) + tuple(region)


class Problem:
    """One (shape, window, inputs) on the device, and the calls on it."""

    def __init__(self, shape, region, y, da, gamma, beta, tile_stats=None):
        from tests.ln_cases import ln_geometry
        self.shape, self.region = shape, region
        self.y, self.da, self.gamma, self.beta = (t.cuda().contiguous() for t in (y, da, gamma, beta))
        self.ts = None if tile_stats is None else tile_stats.cuda().contiguous()
        B, H, W, C = shape
        self.G = ln_geometry(B, H * W, C).G
        self.dims = (B, H * W, C) + region_args(region, W)

    def ws(self, lib):
        return torch.zeros(lib.L.sgg_layernorm_hwc_elu_workspace_bytes(*self.dims[:3]), dtype=torch.uint8, device="cuda")

    def fwd(self, lib, fmt, ts=None, ws=None, a=None):
        B = self.shape[0]
        a = torch.full(self.shape, float("nan"), device="cuda") if a is None else a
        stats, amax = torch.full((B, 2), float("nan"), device="cuda"), torch.zeros(1, device="cuda")
        ws = self.ws(lib) if ws is None else ws
        lib.call("sgg_layernorm_hwc_elu_fwd", self.y, self.gamma, self.beta, a, stats, amax, ts, 0 if ts is None else ts.shape[1],
                 *self.dims, fmt, ws, ws.numel())
        return {"a": a, "stats": stats, "amax": amax, "workspace": ws}

    def bwd(self, lib, stats, fmt, deferred, ws=None, dy=None):
        C = self.shape[3]
        dy = torch.full(self.shape, float("nan"), device="cuda") if dy is None else dy
        grads = [torch.full((C,), float("nan"), device="cuda") for _ in range(3)]
        amax, pq = torch.zeros(1, device="cuda"), torch.zeros(2, device="cuda")
        ws = self.ws(lib) if ws is None else ws
        lib.call("sgg_layernorm_hwc_elu_bwd", self.y, self.da, self.gamma, self.beta, stats, dy, *([None] * 3 if deferred else grads), amax,
                 *self.dims, fmt, pq, ws, ws.numel())
        return {"dy": dy, "dgamma": grads[0], "dbeta": grads[1], "dbias_prev": grads[2], "amax": amax, "pq": pq, "workspace": ws}

    def finalize_deferred(self, lib, stats, out):
        from sgg_amd.lib import LnFinalizeDesc
        B, HW, C = self.dims[:3]
        d = LnFinalizeDesc(out["workspace"].data_ptr(), self.gamma.data_ptr(), stats.data_ptr(), out["dgamma"].data_ptr(),
                           out["dbeta"].data_ptr(), out["dbias_prev"].data_ptr(), B, HW, C,
                           HW if self.region is None else self.region[2] * self.region[3])
        lib.call("sgg_layernorm_hwc_bwd_finalize", ctypes.addressof(d), 1)
        torch.cuda.synchronize()          # (d lives until the launch has read it)


def problems():
    from tests import ln_cases
    from tests.test_layernorm_geometry_gpu import inputs
    from tests.test_presplit_gpu import LN_SHAPES
    rnd = lambda shape, seed, scale=1.0: torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32) * scale
    for case in ln_cases.CASES:
        yield "ln_cases", Problem(case.shape, case.region, *inputs(case))
    kernels_shapes = [(s, None) for s in ((2, 8, 8, 32), (3, 7, 7, 64), (2, 16, 16, 512), (2, 40, 40, 32), (1, 4, 4, 256))]
    kernels_shapes += [((2, 16, 16, 32), (1, 1, 15, 15)), ((2, 112, 112, 32), (1, 1, 111, 111)), ((1, 224, 224, 32), (3, 3, 221, 221)),
                       ((3, 12, 12, 128), (2, 3, 9, 7)), ((2, 8, 8, 512), (0, 0, 8, 7))]
    for shape, region in kernels_shapes:          # test_layernorm_elu, test_layernorm_elu_valid_region
        C = shape[3]
        y, da = rnd(shape, 7, 2.0) + 0.3, rnd(shape, 10)
        if region is not None:
            inside = torch.zeros((1,) + shape[1:3] + (1,), dtype=torch.bool)
            inside[:, region[0]:region[0] + region[2], region[1]:region[1] + region[3]] = True
            y, da = torch.where(inside, y, torch.full(shape, 1e6)), torch.where(inside, da, torch.full(shape, -1e6))
        yield "test_kernels", Problem(shape, region, y, da, 1.0 + rnd((C,), 8, 0.2), rnd((C,), 9, 0.2))
    for shape, region in LN_SHAPES:
        C = shape[3]
        yield "test_presplit", Problem(shape, region, rnd(shape, 1) * 1.7 + 0.3, rnd(shape, 2), 1.0 + rnd((C,), 3, 0.2), rnd((C,), 4, 0.2))
    shape = (2, 6, 8, 32)
    y = rnd(shape, 1) * 1.7 + 0.3
    rows = []
    for plane in y.reshape(2, -1).double():
        rows.append([[p.numel(), float(p.mean()), float(((p - p.mean()) ** 2).sum()), float((p - p.mean()).abs().max())]
                     for p in plane.split([512, 640, 384])])
    yield "tile_partials", Problem(shape, None, y, rnd(shape, 2), 1.0 + rnd((32,), 3, 0.2), rnd((32,), 4, 0.2),
                                   torch.tensor(rows, dtype=torch.float64).float())


def bits_leg(libs):
    out, launches, nprob = {}, 0, {}

    def run(what, fn):
        """fn(lib) -> {name: buffer} on fresh buffers per library; the buffers are compared.  Returns both results."""
        nonlocal launches
        res = []
        for lib in libs:
            res.append(fn(lib))
            torch.cuda.synchronize()
        for k in res[0]:
            out["%s.%s" % (what, k)] = out.get("%s.%s" % (what, k), 0) + AB.diff_bits(res[0][k], res[1][k])
        launches += 1
        return res

    for group, P in problems():
        nprob[group] = nprob.get(group, 0) + 1
        B, H, W, C = P.shape
        f32 = run("fwd[f32, own statistics]", lambda lib: P.fwd(lib, 0))
        run("fwd[pre-split, own statistics]", lambda lib: P.fwd(lib, 1))
        if P.region is None:
            # the partials of each library's own statistics pass (compared above as part of the workspace), or the host-made ones
            ts = [P.ts if P.ts is not None else r["workspace"].view(torch.float32)[:B * P.G * 4].reshape(B, P.G, 4).clone() for r in f32]
            by = dict(zip(libs, ts))
            run("fwd[f32, tile_stats]", lambda lib: P.fwd(lib, 0, by[lib]))
            run("fwd[pre-split, tile_stats]", lambda lib: P.fwd(lib, 1, by[lib]))

            def finalize(lib):
                stats, amax = torch.full((B, 2), float("nan"), device="cuda"), torch.zeros(1, device="cuda")
                lib.call("sgg_layernorm_hwc_finalize", by[lib], by[lib].shape[1], P.gamma, P.beta, stats, amax, B, H * W, C)
                return {"stats": stats, "amax": amax}
            run("finalize", finalize)
        stats = f32[0]["stats"]          # (the parent's: the same input for both libraries)

        def presplit(lib):
            o = torch.full(P.shape, float("nan"), device="cuda")
            lib.call("sgg_presplit16", f32[0]["a"], o, f32[0]["a"].numel(), f32[0]["amax"])
            return {"out": o}
        run("presplit16", presplit)
        for fmt, tag in ((0, "f32"), (1, "pre-split")):
            run("bwd[%s, immediate finalize]" % tag, lambda lib: P.bwd(lib, stats, fmt, False))

            def deferred(lib):
                o = P.bwd(lib, stats, fmt, True)
                P.finalize_deferred(lib, stats, o)
                return o
            run("bwd[%s, deferred finalize] + bwd_finalize" % tag, deferred)
        if P.region is None:
            def sums(lib):
                means, ws = torch.full((B, 2), float("nan"), device="cuda"), P.ws(lib)
                lib.call("sgg_layernorm_hwc_elu_bwd_sums", P.y, P.da, P.gamma, P.beta, stats, means, None, None, None, B, H * W, C, ws, ws.numel())
                return {"means": means, "workspace": ws}
            means = run("bwd_sums", sums)[0]["means"]
            if C == 32:
                gen = torch.Generator().manual_seed(1)
                x, w = torch.randn((B, H, W, 3), generator=gen).cuda(), (torch.randn((3, 3, 3, 32), generator=gen) * 0.2).cuda()

                def wgrad(lib):
                    dw = torch.full((3, 3, 3, 32), float("nan"), device="cuda")
                    ws = torch.zeros(lib.L.sgg_conv2d_nhwc_wgrad_workspace_bytes(B, H, W, 3, H, W, 32, 3, 3), dtype=torch.uint8, device="cuda")
                    lib.call("sgg_conv2d_nhwc_wgrad_c3_ln", x, P.y, P.da, P.gamma, P.beta, stats, means, dw, B, H, W, 1, 1, ws, ws.numel())
                    return {"dw": dw, "workspace": ws}
                run("conv_c3_wgrad_ln", wgrad)

                def dgrad(lib):
                    dx = torch.full((B, H, W, 3), float("nan"), device="cuda")
                    lib.call("sgg_conv2d_nhwc_dgrad_c3_ln", P.y, P.da, P.gamma, P.beta, stats, means, w, dx, B, H, W, 1, 1)
                    return {"dx": dx}
                run("conv_c3_dgrad_ln", dgrad)
        del P, f32
        torch.cuda.empty_cache()
    return {"problems": nprob, "launch_pairs": launches, "differing_bits": out, "ok": not any(out.values())}


def timing_leg(libs, names, repeats, burst=10):
    gen = torch.Generator(device="cuda").manual_seed(11)
    fns = [{} for _ in libs]
    B = TIMING_B
    for (H, W, C), region in [(s, None) for s in TIMING_SHAPES] + [TIMING_MASKED]:
        shape = (B, H, W, C)
        y, da = (torch.randn(shape, generator=gen, device="cuda") * s + o for s, o in ((2.0, 0.3), (1.0, 0.0)))
        P = Problem(shape, region, y, da, 1.0 + 0.2 * torch.randn(C, generator=gen, device="cuda"), 0.2 * torch.randn(C, generator=gen, device="cuda"))
        del y, da
        out, ws = torch.empty(shape, device="cuda"), P.ws(libs[0])
        stats = P.fwd(libs[0], 0, ws=ws, a=out)["stats"]
        ts = ws.view(torch.float32)[:B * P.G * 4].reshape(B, P.G, 4).clone()
        st_o, amax, pq = torch.empty((B, 2), device="cuda"), torch.zeros(1, device="cuda"), torch.zeros(2, device="cuda")
        tag = "%dx%dx%d%s" % (H, W, C, "" if region is None else "_window")

        def fwd(lib, fmt, ts, P=P, out=out, ws=ws, st_o=st_o, amax=amax):
            lib.call("sgg_layernorm_hwc_elu_fwd", P.y, P.gamma, P.beta, out, st_o, amax, ts, 0 if ts is None else ts.shape[1], *P.dims, fmt,
                     ws, ws.numel())

        def bwd(lib, fmt, P=P, out=out, ws=ws, stats=stats, amax=amax, pq=pq):
            lib.call("sgg_layernorm_hwc_elu_bwd", P.y, P.da, P.gamma, P.beta, stats, out, None, None, None, amax, *P.dims, fmt, pq, ws,
                     ws.numel())
        for lib, f in zip(libs, fns):
            f["fwd_f32/" + tag] = lambda lib=lib, fwd=fwd: fwd(lib, 0, None)
            if region is None:          # (tile_stats cover whole planes; the masked pre-split leg runs its own statistics pass)
                f["fwd_presplit_tile_stats/" + tag] = lambda lib=lib, fwd=fwd, ts=ts: fwd(lib, 1, ts)
                f["finalize/" + tag] = lambda lib=lib, P=P, ts=ts, st_o=st_o, amax=amax, d=(B, H * W, C): lib.call(
                    "sgg_layernorm_hwc_finalize", ts, ts.shape[1], P.gamma, P.beta, st_o, amax, *d)
            else:
                f["fwd_presplit/" + tag] = lambda lib=lib, fwd=fwd: fwd(lib, 1, None)
            f["bwd_f32_deferred/" + tag] = lambda lib=lib, bwd=bwd: bwd(lib, 0)
            f["bwd_presplit_deferred/" + tag] = lambda lib=lib, bwd=bwd: bwd(lib, 1)
        if (H, W, C) == TIMING_SHAPES[0]:
            x, w = torch.randn((B, H, W, 3), generator=gen, device="cuda"), 0.2 * torch.randn((3, 3, 3, 32), generator=gen, device="cuda")
            means, dw, dx = torch.empty((B, 2), device="cuda"), torch.empty((3, 3, 3, 32), device="cuda"), torch.empty((B, H, W, 3), device="cuda")
            wws = torch.empty(libs[0].L.sgg_conv2d_nhwc_wgrad_workspace_bytes(B, H, W, 3, H, W, 32, 3, 3), dtype=torch.uint8, device="cuda")
            libs[0].call("sgg_layernorm_hwc_elu_bwd_sums", P.y, P.da, P.gamma, P.beta, stats, means, None, None, None, B, H * W, C, ws, ws.numel())
            for lib, f in zip(libs, fns):
                f["bwd_sums+conv_c3_wgrad_ln/" + tag] = lambda lib=lib, P=P, ws=ws, stats=stats, means=means, x=x, dw=dw, wws=wws, d=(B, H, W, C): (
                    lib.call("sgg_layernorm_hwc_elu_bwd_sums", P.y, P.da, P.gamma, P.beta, stats, means, None, None, None, d[0], d[1] * d[2], d[3],
                             ws, ws.numel()),
                    lib.call("sgg_conv2d_nhwc_wgrad_c3_ln", x, P.y, P.da, P.gamma, P.beta, stats, means, dw, d[0], d[1], d[2], 1, 1, wws, wws.numel()))
                f["conv_c3_dgrad_ln/" + tag] = lambda lib=lib, P=P, stats=stats, means=means, w=w, dx=dx, d=(B, H, W): lib.call(
                    "sgg_conv2d_nhwc_dgrad_c3_ln", P.y, P.da, P.gamma, P.beta, stats, means, w, dx, d[0], d[1], d[2], 1, 1)
    legs = list(fns[0])
    res = {"batch": B, "burst": burst, "repeats": repeats, "order": "%s first in even repetitions, %s first in odd ones" % tuple(names),
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
    rec = {"metric": "ln_refactor_ab", "parent": os.path.basename(args.parent), "new": os.path.basename(args.new or LIB_PATH),
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
