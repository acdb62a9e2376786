"""bench_eval.py - R@50 / R@100 evaluation throughput: SceneGraphGAN.test() (TEST_BATCH_SIZE images per encoder pass, all
N = 8 x TEST_BATCH_SIZE samples of them as one head pass) against the reference's protocol (train.py:297-335: per image 8 passes
of TEST_BATCH_SIZE copies through build_generator / build_discriminator), same seeded weights, images and noise.

    python scripts/bench_eval.py [--batch-size 64] [--size 224] [--vocab 1000] [--images 64] [--legacy-images 4]

Prints ONE JSON line: images/s and ms per image of both legs and the speedup, the peak device memory of the batched evaluation,
and the agreement of the legs on the legacy leg's images (fraction of equal tokens; tokens equal wherever the legacy top-2 logit
margin exceeds 4 x the logit tolerance; max critic-score difference against 1e-4 + 1e-4 * max|score|).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def legacy_eval(gan, items, K):
    """The per-image protocol the batched path replaced: 8 passes of TEST_BATCH_SIZE copies of the image, each through a full
    encoder of G and of D (for_backward=True, as build_* run it).  Same noise stream as test()."""
    TB, passes = gan.TEST_BATCH_SIZE, gan.TEST_BATCH_MULTIPLIER
    gen = torch.Generator().manual_seed(gan.seed + 123)
    toks = torch.empty((TB, 3), dtype=torch.int64, device=gan.device)
    out = []
    for image, _ in items:
        images = image.unsqueeze(0).expand(TB, -1, -1, -1).contiguous().to(gan.device)
        fakes, scores, margins = [], [], []
        for _ in range(passes):
            noise = torch.randn((TB, 512), generator=gen).to(gan.device)
            logits = gan.g.build_generator(images, False, noise)
            K.argmax_rows(logits, toks.view(-1))
            top = logits.topk(2, dim=-1).values
            margins.append((top[..., 0] - top[..., 1]).cpu().numpy())
            mx = float(logits.abs().max())
            d = gan.d.build_discriminator(logits, images, False)
            fakes.append(toks.cpu().numpy().copy())
            scores.append(d.cpu().numpy().mean(axis=1).reshape(-1))
        out.append({"tokens": np.concatenate(fakes), "scores": np.concatenate(scores), "margins": np.concatenate(margins),
                    "max_abs_logit": mx})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--vocab", type=int, default=1000)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--legacy-images", type=int, default=4)
    ap.add_argument("--workdir", default="/tmp/sgg_bench_eval")
    args = ap.parse_args()
    import train as T
    from sgg_amd.api import kernels_for
    B, S, V = args.batch_size, args.size, args.vocab
    gan = T.SceneGraphGAN(os.path.join(args.workdir, "ck"), os.path.join(args.workdir, "logs"), None, None, None, None, None,
                          critic_iters=1, batch_size=B, lambda_=10, resume=False, synthetic=(B, S, V))
    K = kernels_for(gan.device)
    g = torch.Generator().manual_seed(4242)
    items = [(torch.randn((S, S, 3), generator=g), [[0, 0, 0]]) for _ in range(max(args.images, args.legacy_images))]
    TB, N = gan.TEST_BATCH_SIZE, gan.TEST_BATCH_MULTIPLIER * gan.TEST_BATCH_SIZE
    # warm-up: both networks and their buffers at the test batch size, one image batch each way
    gan.test(items=items[:TB], out_path=None)
    legacy_eval(gan, items[:1], K)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    _, det = gan.test(items=items[:args.images], out_path=None, return_details=True)
    torch.cuda.synchronize()
    t_b = time.perf_counter() - t0
    peak = torch.cuda.max_memory_allocated()
    t0 = time.perf_counter()
    leg = legacy_eval(gan, items[:args.legacy_images], K)
    torch.cuda.synchronize()
    t_l = time.perf_counter() - t0
    eq, n_tok, guarded_ok, n_guarded, sdiff, smax = 0, 0, True, 0, 0.0, 0.0
    for d, l in zip(det, leg):
        same = d["tokens"] == l["tokens"]
        eq, n_tok = eq + int(same.sum()), n_tok + same.size
        resolved = l["margins"] > 4.0 * (1e-5 + 1e-5 * l["max_abs_logit"])
        n_guarded += int(resolved.sum()) * 3
        guarded_ok &= bool(same[resolved].all())
        sdiff = max(sdiff, float(np.abs(d["scores"] - l["scores"]).max()))
        smax = max(smax, float(np.abs(l["scores"]).max()))
    ips_b, ips_l = args.images / t_b, args.legacy_images / t_l
    rec = {"metric": "eval_images_per_s", "batch_size": B, "size": S, "vocab": V, "test_batch_size": TB, "samples_per_image": N,
           "batched": {"images": args.images, "images_per_s": round(ips_b, 3), "ms_per_image": round(1e3 / ips_b, 3),
                       "peak_mem_gb": round(peak / 2 ** 30, 3), "mem_before_gb": round(base / 2 ** 30, 3)},
           "legacy": {"images": args.legacy_images, "images_per_s": round(ips_l, 3), "ms_per_image": round(1e3 / ips_l, 3)},
           "speedup": round(ips_b / ips_l, 2),
           "agreement": {"token_equal_fraction": eq / max(1, n_tok), "tokens_equal_where_margin_resolved": guarded_ok,
                         "resolved_tokens": n_guarded, "max_score_diff": sdiff, "score_tol": 1e-4 + 1e-4 * smax,
                         "scores_ok": sdiff <= 1e-4 + 1e-4 * smax},
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
