"""CPU: the score-function update with S sampled triples per image (csrc/score.hip's sgg_sample_rows_multi /
sgg_score_advantage_multi / sgg_score_rows_multi / sgg_score_summary_multi, GanStep.set_estimator(samples=S), train.py
--score_samples) in fp64 on the kernel-level reference: the estimator's expectation over all sample tuples is the true gradient for
every baseline (by enumeration), the restatement's known answers, the host logic of the step against autograd on the surrogate
    -(1/(B S)) sum_{b,s} A_sb.detach() sum_t log_softmax(x)[a_sbt] - (w/B) sum H,
accumulation, the guard and the weight average, the unchanged samples = 1 path, and train.py on the reference kernels.

Bounds: those of tests/test_score_cpu.py (both sides fp64, differing by summation order): GRAD_RTOL on gradients where the issue
names it, 1e-9 on parameters after Adam, 1e-8 for accumulated against the calls' own sum, 1e-12 for the enumeration."""
import itertools
import json

import numpy as np
import pytest
import torch

import sgg_amd  # noqa: F401
from oracle import sgg_oracle as O
from sgg_amd.params import T_STEPS
from sgg_amd.step import GanStep
from tests import relax_ref as RR
from tests import score_multi_ref as MR
from tests import score_ref as SR
from tests import xent_ref as XR
from tests.test_relax_cpu import SEED, _states
from tests.test_score_cpu import NEW, RELAX, ScoreRefKernels
from tests.test_step_cpu import rel_err
from tests.test_xent_cpu import cpu_train  # noqa: F401  (the fixture)
from tests.tolerances import GRAD_RTOL

DT = torch.float64
V, B = 11, 2
MULTI = ("sample_rows_multi", "score_advantage_multi", "score_rows_multi", "score_summary_multi")
HARD_GUMBEL = ("gumbel", 1.0, SEED, True)


class ScoreMultiRefKernels(ScoreRefKernels):
    """ScoreRefKernels with torch versions of the four multi-sample entry points in the arithmetic of their tensors; every call is
    recorded (`calls`, arguments in `multi_log`)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.multi_log, self.gathers = [], []

    def embed_gather_fwd(self, idx, W, out):
        self.gathers.append(int(idx.numel()))
        return super().embed_gather_fwd(idx, W, out)

    def sample_rows_multi(self, x, tok, seed=0, draw=0):
        self.calls.append("sample_rows_multi")
        S = tok.shape[0]
        self.multi_log.append({"op": "sample", "S": int(S), "seed": int(seed), "draw": int(draw)})
        assert 1 <= S <= 16 and 0 <= int(draw) < 2 ** 56 and tok.numel() == S * x.numel() // x.shape[-1]
        for s in range(S):
            tok[s].copy_(torch.argmax(self._noisy(x, True, seed, MR.sample_draw(draw, s)), dim=-1).reshape(tok[s].shape))
        return tok

    def score_advantage_multi(self, d_out, samples, baseline="image", adv=None, out2=None):
        self.calls.append("score_advantage_multi")
        self.multi_log.append({"op": "advantage", "S": int(samples), "baseline": baseline})
        N, S = d_out.shape[0], int(samples)
        assert N % S == 0
        r = d_out.mean(dim=1)
        if baseline == "rloo":
            assert N >= 2
            a = r - (r.sum() - r) / (N - 1)
        elif baseline == "image":
            assert S >= 2
            rs = r.view(S, N // S)
            a = (rs - (rs.sum(dim=0, keepdim=True) - rs) / (S - 1)).reshape(N)
        else:
            assert baseline == "none"
            a = r.clone()
        if adv is None:
            adv = torch.zeros_like(r)
        adv.copy_(a)
        if out2 is not None:
            out2[0], out2[1] = r.mean(), (a * a).mean()
        return adv

    def score_rows_multi(self, x, tok, adv=None, group=1, coef=1.0, ent_coef=0.0, accumulate=False, dx=None, logp=None, ent=None):
        self.calls.append("score_rows_multi")
        S = tok.shape[0]
        self.multi_log.append({"op": "rows", "S": int(S), "group": int(group), "coef": float(coef), "ent_coef": float(ent_coef),
                               "accumulate": bool(accumulate)})
        assert dx is None or dx.data_ptr() != x.data_ptr(), "dx must not alias x"
        Vx = x.shape[-1]
        z = x.reshape(-1, Vx)
        R = z.shape[0]
        t = tok.reshape(S, R)
        assert R % group == 0 and (adv is None or adv.numel() >= S * (R // group))
        rows = torch.arange(R)
        logq = torch.log_softmax(z, dim=-1)
        p = torch.exp(logq)
        H = -(p * logq).sum(dim=-1)
        g = float(ent_coef) * p * (logq + H[:, None])
        lp = torch.zeros(S, R, dtype=z.dtype)
        for s in range(S):
            valid = (t[s] >= 0) & (t[s] < Vx)
            safe = torch.where(valid, t[s], torch.zeros_like(t[s]))
            w = torch.full((R,), float(coef), dtype=z.dtype) if adv is None else float(coef) * adv.reshape(-1)[s * (R // group) + rows // int(group)]
            w = w * valid.to(z.dtype)
            hot = torch.zeros_like(p)
            hot[rows, safe] = 1.0
            g = g + w[:, None] * (p - hot)
            lp[s] = torch.where(valid, logq[rows, safe], torch.zeros_like(H))
        if ent is not None:
            ent.copy_(H.reshape(ent.shape))
        if logp is not None:
            logp.copy_(lp.reshape(logp.shape))
        if dx is not None:
            d = dx.view(-1, Vx)
            if accumulate:
                d += g
            else:
                d.copy_(g)
        return dx

    def score_summary_multi(self, logp, ent, out2=None):
        self.calls.append("score_summary_multi")
        if out2 is None:
            out2 = torch.zeros(2, dtype=logp.dtype)
        out2[0], out2[1] = logp.mean(), ent.mean()
        return out2


# ---- the estimator is the gradient ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("baseline", ["image", "rloo", "none"])
@pytest.mark.parametrize("Bn", [1, 2])
def test_expectation_over_all_sample_tuples_is_the_gradient_by_enumeration(Bn, baseline):
    """S = 2 samples of T = 2 tokens over V = 3 for B images: the restatement's dx averaged over all 3^(S B T) joint outcomes with their
    probabilities equals autograd's gradient of -(1/B) sum_b E[r_b] - (0.3/B) sum H; no baseline changes the expectation.  With
    "image" the S advantages of every image sum to zero in every outcome."""
    S, T, Vn, w = 2, 2, 3, 0.3
    g = np.random.RandomState(17 + Bn)
    x = g.standard_normal((Bn, T, Vn))
    table = 2.0 * g.standard_normal((Bn, Vn, Vn, T))              # the critic's T outputs for image b's tokens (a0, a1)
    p = np.exp(x - XR.lse64(x)[..., None])
    mean, total, worst_sum = np.zeros((Bn * T, Vn)), 0.0, 0.0
    for flat in itertools.product(range(Vn), repeat=S * Bn * T):
        tok = np.array(flat).reshape(S, Bn, T)
        prob = float(np.prod([p[b, t, tok[s, b, t]] for s in range(S) for b in range(Bn) for t in range(T)]))
        d_out = np.stack([table[b, tok[s, b, 0], tok[s, b, 1]] for s in range(S) for b in range(Bn)])
        adv, _ = MR.score_advantage_multi(d_out, S, baseline)
        if baseline == "image":
            worst_sum = max(worst_sum, float(np.abs(adv.reshape(S, Bn).sum(axis=0)).max()))
        mean += prob * MR.score_rows_multi(x.reshape(-1, Vn), tok.reshape(S, -1), adv, group=T, coef=1.0 / (Bn * S), ent_coef=w / Bn)["dx"]
        total += prob
    assert abs(total - 1.0) < 1e-12 and worst_sum < 1e-14
    xt = torch.from_numpy(x).requires_grad_(True)
    logq = torch.log_softmax(xt, dim=-1)
    q = torch.exp(logq)
    r = torch.from_numpy(table).mean(dim=-1)
    expected_r = torch.einsum("bi,bj,bij->b", q[:, 0], q[:, 1], r)
    H = -(q * logq).sum(dim=-1)
    (-(expected_r.sum() / Bn) - (w / Bn) * H.sum()).backward()
    err = float(np.abs(mean - xt.grad.numpy().reshape(-1, Vn)).max())
    print("E[dx] against autograd (B %d, %s): %.3e" % (Bn, baseline, err))
    assert err <= 1e-12
    assert float(np.abs(xt.grad.numpy()).max()) > 1e-2


# ---- known answers -----------------------------------------------------------------------------------------------------------------------
def test_restatement_known_answers():
    # rewards of S = 2 samples of B = 3 images: [[2, -1, 5], [4, 1, -3]]
    d = np.array([[1.0, 3.0], [0.0, -2.0], [4.0, 6.0], [3.0, 5.0], [1.0, 1.0], [-2.0, -4.0]])
    adv, out2 = MR.score_advantage_multi(d, 2, "none")
    assert np.array_equal(adv, [2.0, -1.0, 5.0, 4.0, 1.0, -3.0]) and np.allclose(out2, [8.0 / 6.0, 56.0 / 6.0], rtol=0, atol=1e-15)
    adv, _ = MR.score_advantage_multi(d, 2, "image")               # S = 2: each sample against the other one of its image
    assert np.allclose(adv, [-2.0, -2.0, 8.0, 2.0, 2.0, -8.0], rtol=0, atol=1e-15)
    adv, _ = MR.score_advantage_multi(d, 2, "rloo")                # against the mean of the other five
    assert np.allclose(adv, [2.0 - 6.0 / 5, -1.0 - 9.0 / 5, 5.0 - 3.0 / 5, 4.0 - 4.0 / 5, 1.0 - 7.0 / 5, -3.0 - 11.0 / 5], rtol=0, atol=1e-15)
    # S = 1 is score_ref's (none, rloo)
    for base in ("none", "rloo"):
        a1, o1 = MR.score_advantage_multi(d, 1, base)
        a0, o0 = SR.score_advantage(d, base)
        assert np.array_equal(a1, a0) and np.array_equal(o1, o0)
    # B = 1 with the per-image baseline: three samples of one image, rewards 2, -1, 5
    adv, out2 = MR.score_advantage_multi(d[:3], 3, "image")
    assert np.allclose(adv, [0.0, -4.5, 4.5], rtol=0, atol=1e-15) and abs(adv.sum()) < 1e-15 and np.allclose(out2, [2.0, 13.5], rtol=0, atol=1e-14)
    with pytest.raises(AssertionError):
        MR.score_advantage_multi(d, 1, "image")
    with pytest.raises(AssertionError):
        MR.score_advantage_multi(d[:1], 1, "rloo")
    # rows.  S = 1 is score_ref's on rows whose token is valid
    g = np.random.RandomState(5)
    x = 2.0 * g.standard_normal((4, 5))
    tok1 = np.array([[1, 0, 4, 2]])
    a = np.array([0.5, -1.5])
    one = MR.score_rows_multi(x, tok1, a, group=2, coef=0.5, ent_coef=0.4)
    ref = SR.score_rows(x, tok1[0], a, group=2, coef=0.5, ent_coef=0.4)
    assert np.abs(one["dx"] - ref["dx"]).max() < 1e-15 and np.array_equal(one["logp"][0], ref["logp"]) and np.array_equal(one["ent"], ref["ent"])
    # S samples are the sum of S single-sample calls without the entropy term, plus it once
    tok = np.array([[1, 0, 4, 2], [1, 3, 0, 2], [2, 3, 4, 0]])                  # row 0: tok[1] = tok[0], a duplicate token
    adv = g.standard_normal(3 * 2)
    res = MR.score_rows_multi(x, tok, adv, group=2, coef=0.25, ent_coef=0.4)
    parts = sum(SR.score_rows(x, tok[s], adv[2 * s:2 * s + 2], group=2, coef=0.25)["dx"] for s in range(3))
    assert np.abs(res["dx"] - (parts + SR.score_rows(x, tok[0], None, coef=0.0, ent_coef=0.4)["dx"])).max() < 1e-15
    assert float(np.abs(res["dx"].sum(axis=1)).max()) < 1e-15
    # the duplicate counts twice: at its index the two one-hot terms add up
    p = np.exp(x - XR.lse64(x)[:, None])
    w0, w1, w2 = 0.25 * adv[0], 0.25 * adv[2], 0.25 * adv[4]
    noent = MR.score_rows_multi(x, tok, adv, group=2, coef=0.25)["dx"]
    assert abs(noent[0, 1] - ((w0 + w1 + w2) * p[0, 1] - (w0 + w1))) < 1e-15 and abs(noent[0, 2] - ((w0 + w1 + w2) * p[0, 2] - w2)) < 1e-15
    # an invalid token drops that sample's term alone: logp 0 there, the other samples, the entropy term and the row's store stay
    bad = tok.copy()
    bad[1, 2] = 5
    bad[2, 3] = -1
    got = MR.score_rows_multi(x, bad, adv, group=2, coef=0.25, ent_coef=0.4)
    assert got["logp"][1, 2] == 0.0 and got["logp"][2, 3] == 0.0 and np.array_equal(got["ent"], res["ent"])
    assert np.array_equal(got["dx"][:2], res["dx"][:2]) and np.array_equal(np.delete(got["logp"], [1 * 4 + 2, 2 * 4 + 3]), np.delete(res["logp"], [6, 11]))
    hot = np.zeros(5)
    hot[0] = 1.0
    assert np.abs(got["dx"][2] - (res["dx"][2] - 0.25 * adv[3] * (p[2] - hot))).max() < 1e-15
    old = g.standard_normal((4, 5))
    acc = MR.score_rows_multi(x, bad, adv, group=2, coef=0.25, ent_coef=0.4, accumulate=True, dx=old)["dx"]
    assert np.abs(acc - (old + got["dx"])).max() < 1e-15
    # the sampler is relax_hard_ref's at the draw number draw | (s << 56), and a Gumbel-max sample of softmax(x)
    assert MR.sample_draw(77, 0) == 77 and MR.sample_draw(77, 3) == 77 + 3 * 2 ** 56
    t, margin = MR.sample_rows_multi(x, 3, SEED, 77)
    for s in range(3):
        gum = RR.gumbel(RR.uniforms(SEED, 77 + s * 2 ** 56, 4, 5))
        assert np.array_equal(t[s], (x + gum).argmax(axis=1)) and (margin[s] > 0).all()
    assert not np.array_equal(t[0], t[1]) or not np.array_equal(t[0], t[2]), "the samples are different draws"
    assert np.allclose(MR.score_summary_multi([1.0, 2.0, 6.0, 3.0], [0.5, 1.5]), [3.0, 1.0], rtol=0, atol=1e-15)


def test_torch_entry_points_follow_the_restatement():
    K = ScoreMultiRefKernels()
    g = np.random.RandomState(3)
    x, S = 3.0 * g.standard_normal((6, 7)), 3
    d = g.standard_normal((S * 2, 3))
    tok = torch.zeros(S, 6, dtype=torch.int64)
    K.sample_rows_multi(torch.from_numpy(x), tok, seed=SEED, draw=9)
    assert np.array_equal(tok.numpy(), MR.sample_rows_multi(x, S, SEED, 9)[0])
    tok[1, 2], tok[2, 0], tok[1, 4] = 7, -1, tok[0, 4]
    for baseline in ("image", "rloo", "none"):
        adv, out2 = torch.zeros(S * 2, dtype=DT), torch.zeros(2, dtype=DT)
        K.score_advantage_multi(torch.from_numpy(d), S, baseline, adv=adv, out2=out2)
        a64, o64 = MR.score_advantage_multi(d, S, baseline)
        assert np.abs(adv.numpy() - a64).max() < 1e-14 and np.abs(out2.numpy() - o64).max() < 1e-14
        for acc in (False, True):
            dx0 = g.standard_normal((6, 7))
            dx, logp, ent = torch.from_numpy(dx0.copy()), torch.zeros(S * 6, dtype=DT), torch.zeros(6, dtype=DT)
            K.score_rows_multi(torch.from_numpy(x), tok, adv, group=3, coef=0.5, ent_coef=0.2, accumulate=acc, dx=dx, logp=logp, ent=ent)
            ref = MR.score_rows_multi(x, tok.numpy(), a64, group=3, coef=0.5, ent_coef=0.2, accumulate=acc, dx=dx0)
            assert np.abs(dx.numpy() - ref["dx"]).max() < 1e-14 and np.abs(logp.numpy() - ref["logp"].reshape(-1)).max() < 1e-14
            assert np.abs(ent.numpy() - ref["ent"]).max() < 1e-14
        assert np.abs(K.score_summary_multi(logp, ent).numpy() - MR.score_summary_multi(ref["logp"], ref["ent"])).max() < 1e-14


# ---- host logic in fp64: autograd on the surrogate ---------------------------------------------------------------------------------------
def _fresh(S=32, rows=B, reducer=None, K=None, relax=HARD_GUMBEL, score=None, samples=None):
    gp, dp_ = _states(S)
    gs = GanStep(K if K is not None else ScoreMultiRefKernels(), V, S, rows, g_state=gp, d_state=dp_, dtype=DT, reducer=reducer)
    if relax is not None:
        gs.set_relaxation(*relax[:3], **({"hard": relax[3]} if len(relax) > 3 else {}))
    if score is not None:
        gs.set_estimator("score", *score, **({"samples": samples} if samples is not None else {}))
    return gs, gp, dp_


def oracle_g_score_multi(gp, dp_, images, noise, seed, draw, S, baseline="image", w_ent=0.0, labels=None, w=0.0, tok=None):
    """generator_forward -> S Gumbel-max token sets (draw | (s << 56); or `tok` [S, B, 3] as given) -> rewards from
    discriminator_forward on their one-hot rows against the images repeated S times (constants) -> the surrogate's gradients.
    Returns a dict: grads of gp, tok [S, B, 3], margin, numbers = (mean reward, mean A^2, mean log p per sampled token, mean H per
    token), d_mean, max_adv, rewards [S, B]."""
    gp = {k: v.clone().requires_grad_(True) for k, v in gp.items()}
    fake = O.generator_forward(gp, images, noise)
    Bn, Vn = fake.shape[0], fake.shape[-1]
    own, margin = MR.sample_rows_multi(fake.detach().reshape(-1, Vn).numpy(), S, seed, draw)
    if tok is None:
        tok = torch.from_numpy(own).view(S, Bn, T_STEPS)
    with torch.no_grad():
        hot = torch.nn.functional.one_hot(tok.reshape(S * Bn, T_STEPS), Vn).to(fake.dtype)
        d = O.discriminator_forward(dp_, hot, images.repeat(S, 1, 1, 1)).reshape(S * Bn, -1)
        A, _ = MR.score_advantage_multi(d.numpy(), S, baseline)
        A = torch.from_numpy(A).to(fake.dtype).view(S, Bn)
        r = d.mean(dim=1).view(S, Bn)
    logq = torch.log_softmax(fake, dim=-1)
    logp = torch.stack([logq.gather(-1, tok[s].unsqueeze(-1)).squeeze(-1) for s in range(S)])        # [S, B, 3]
    H = -(torch.exp(logq) * logq).sum(dim=-1)
    cost = -(A.detach() * logp.sum(dim=2)).sum() / (Bn * S) - (w_ent / Bn) * H.sum()
    if w > 0.0:
        cost = cost + w * (-logq.gather(-1, labels.unsqueeze(-1)).sum() / Bn)
    return {"grads": O._grads(cost, gp), "tok": tok, "own_tok": torch.from_numpy(own).view(S, Bn, T_STEPS), "margin": float(margin.min()),
            "d_mean": float(d.mean()), "max_adv": float(A.abs().max()), "rewards": r,
            "numbers": [float(r.mean()), float((A * A).mean()), float(logp.mean().detach()), float(H.mean().detach())]}


@pytest.mark.parametrize("baseline,w_ent,w_mle", [("image", 0.0, 0.0), ("image", 0.05, 0.0), ("rloo", 0.05, 0.0), ("none", 0.0, 0.0),
                                                   ("image", 0.05, 0.1)])
def test_generator_step_with_three_samples_matches_autograd_on_the_surrogate(baseline, w_ent, w_mle):
    Sz, S = 32, 3
    images, labels, _ = O.synth_batch(B, Sz, V, dtype=DT)
    noise = O.synth_noise(B, 1, DT)
    gs, gp, dp_ = _fresh(Sz, score=(baseline, w_ent), samples=S)
    assert gs.estimator == {"kind": "score", "baseline": baseline, "entropy_weight": w_ent, "samples": S}
    d_grads0 = gs.D.grad_flat.clone()
    kw = {"labels": labels, "mle_weight": w_mle} if w_mle > 0.0 else {}
    ref = oracle_g_score_multi(gp, dp_, images, noise, SEED, 41, S, baseline, w_ent, labels, w_mle)
    gl = gs.generator_step(images, noise, draw=41, **kw)
    K = gs.K
    assert [c for c in K.calls if c in RELAX + NEW + MULTI] == list(MULTI), "one launch each, nothing of the single-sample path"
    assert K.multi_log == [{"op": "sample", "S": S, "seed": SEED, "draw": 41}, {"op": "advantage", "S": S, "baseline": baseline},
                           {"op": "rows", "S": S, "group": T_STEPS, "coef": 1.0 / (B * S), "ent_coef": w_ent / B, "accumulate": False}]
    assert not K.hard_log and K.gathers == [S * B] * T_STEPS, "the tokens enter D as a row gather of S * B rows per step"
    assert [c for c in K.calls if c == "softmax_xent"] == (["softmax_xent"] if w_mle > 0.0 else [])
    assert torch.equal(gs._score_tok, ref["tok"]) and gs._relax_buf is not None and not gs._relax_buf.any(), "no one-hot row was written"
    assert abs(float(gl[3]) - ref["d_mean"]) < 1e-9
    assert np.abs(np.array(gs.score_losses.tolist()) - np.array(ref["numbers"])).max() < 1e-9
    for name, g in ref["grads"].items():
        e = rel_err(gs.G.grads[name], g)
        assert e < GRAD_RTOL and e < 1e-8, "generator grad %s rel err %.3e (%s, w %g)" % (name, e, baseline, w_ent)
    m, v = O.new_adam_state(gp)
    O.tf_adam_step(gp, ref["grads"], m, v, 1)
    for name in gp:
        if not O.is_dead(name):
            assert rel_err(gs.G.arena.views[name], gp[name]) < 1e-9, "generator param after Adam: " + name
    assert torch.equal(gs.D.grad_flat, d_grads0) and gs.D.adam_t == 0, "D's gradient arena was touched"
    # D's head ran forward only: the cell backwards are G's alone, as with one sample
    single, _, _ = _fresh(Sz, score=("rloo", w_ent))
    single.generator_step(images, noise, draw=41, **kw)
    assert K.launches.count("lstm_bwd") == single.K.launches.count("lstm_bwd") > 0
    # ... and the estimators differ
    assert rel_err(single.G.grads["decoder/bias"], ref["grads"]["decoder/bias"]) > 100 * GRAD_RTOL


def test_batch_of_one_image_has_a_baseline_again():
    images, _, _ = O.synth_batch(1, 32, V, dtype=DT)
    noise = O.synth_noise(1, 1, DT)
    gs, gp, dp_ = _fresh(32, rows=1, score=("image", 0.0), samples=4)
    ref = oracle_g_score_multi(gp, dp_, images, noise, SEED, 5, 4, "image")
    gs.generator_step(images, noise, draw=5)
    assert float(gs._score_adv.abs().max()) > 0 and abs(float(gs._score_adv.sum())) < 1e-12
    for name, g in ref["grads"].items():
        assert rel_err(gs.G.grads[name], g) < 1e-8, name


# ---- composition ----------------------------------------------------------------------------------------------------------------------
def test_accumulated_update_is_the_sum_of_its_micro_batches():
    """Two micro-batches of B = 2 with S = 3 samples each (per-image baselines) against the two calls' own sum."""
    Sz = 32
    images, _, _ = O.synth_batch(4, Sz, V, dtype=DT)
    noise = O.synth_noise(4, 1, DT)
    parts, nums = [], []
    for k in range(2):
        one, _, _ = _fresh(Sz, score=("image", 0.05), samples=3)
        one.generator_step(images[2 * k:2 * k + 2], noise[2 * k:2 * k + 2], draw=7 + k)
        parts.append(one.G.grad_flat.clone())
        nums.append(one.score_losses.clone())
    gs, _, _ = _fresh(Sz, score=("image", 0.05), samples=3)
    for k in range(2):
        gs.generator_step(images[2 * k:2 * k + 2], noise[2 * k:2 * k + 2], micro=(k, 2), draw=7 + k)
    err = float((gs.G.grad_flat - (parts[0] + parts[1])).abs().max())
    print("accumulated multi-sample update against the calls' own sum: %.3e" % err)
    assert err < 1e-8 and gs.G.adam_t == 1
    assert float((gs.score_losses_mean - (nums[0] + nums[1]) / 2).abs().max()) < 1e-12
    assert float((parts[0] - parts[1]).abs().max()) > 1e3 * 1e-8


def test_guard_and_average_apply_to_the_multi_sample_updates():
    twin, _, _ = _fresh(score=("image", 0.05), samples=3)
    images, _, _ = O.synth_batch(2, 32, V, dtype=DT)
    twin.generator_step(images, O.synth_noise(2, 0, DT), draw=3)
    norm = float(twin.G.arena.live(twin.G.grad_flat).pow(2).sum().sqrt())
    assert norm > 0
    first, _, _ = _fresh(score=("image", 0.05), samples=3)
    first.set_guard((0.0, norm / 4.0), False)
    first.G.enable_averaging(0.9)
    init = first.G.arena.flat.clone()
    first.generator_step(images, O.synth_noise(2, 0, DT), draw=3)
    r = first.G.guard_report()
    assert r["clipped"] == 1 and abs(r["coef"] - 0.25) < 1e-12 and abs(r["norm"] - norm) < 1e-12 * norm
    assert float((first.G.m_flat - 0.25 * twin.G.m_flat).abs().max()) <= 1e-12 * float(twin.G.m_flat.abs().max())
    avg = first.G.opt["ema"]
    assert avg["updates"] == 1 and not torch.equal(avg["flat"], init) and not torch.equal(avg["flat"], first.G.arena.flat)


# ---- samples = 1 is the path it was -----------------------------------------------------------------------------------------------------
def _one_iteration(gs, **kw):
    images, labels, _ = O.synth_batch(B, 32, V, dtype=DT)
    gs.train_iteration(images, labels, [O.synth_noise(B, i, DT) for i in range(3)], [O.synth_alpha(B, i, DT).reshape(B) for i in range(2)],
                       critic_iters=2, **kw)
    gs.flush()
    return [t.clone() for net in (gs.G, gs.D) for t in (net.arena.flat, net.grad_flat, net.m_flat, net.v_flat)]


def test_samples_1_records_the_single_sample_calls_and_keeps_every_bit():
    """On a kernel set WITHOUT the new entry points (what the step ran on before they existed) and on one with them: the same calls in
    the same order with the same arguments, and every bit of the arenas."""
    base, _, _ = _fresh(K=ScoreRefKernels())
    base.set_estimator("score", "rloo", 0.05)
    want = _one_iteration(base, draws=[1, 2, 3])
    assert [c for c in base.K.calls if c in NEW] == list(NEW)
    for setup in (lambda gs: gs.set_estimator("score", "rloo", 0.05), lambda gs: gs.set_estimator("score", "rloo", 0.05, samples=1),
                  lambda gs: gs.set_estimator("score", None, 0.05, 1),
                  lambda gs: (gs.set_estimator("score", "image", 0.05, samples=4), gs.set_estimator("score", "rloo", 0.05))):
        gs, _, _ = _fresh()
        setup(gs)
        assert gs.estimator == {"kind": "score", "baseline": "rloo", "entropy_weight": 0.05}, "no samples key at S = 1"
        got = _one_iteration(gs, draws=[1, 2, 3])
        assert gs.K.calls == base.K.calls and gs.K.launches == base.K.launches and gs.K.hard_log == base.K.hard_log
        assert gs.K.score_log == base.K.score_log and not gs.K.multi_log
        for a, b in zip(want, got):
            assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    on, _, _ = _fresh(score=("rloo", 0.05), samples=3)
    moved = _one_iteration(on, draws=[1, 2, 3])
    assert not torch.equal(moved[0], want[0]), "three samples move G otherwise"
    assert torch.equal(moved[4], want[4]), "... and the critic's updates of the first iteration keep one sample per image"
    assert [c for c in on.K.calls if c in MULTI] == list(MULTI) and not [c for c in on.K.calls if c in NEW]


def test_set_estimator_refusals():
    gs, _, _ = _fresh()
    for bad in (0, 17, -1, 2.5):
        with pytest.raises(ValueError, match="score_samples"):
            gs.set_estimator("score", "rloo", 0.0, samples=bad)
    with pytest.raises(ValueError, match="image.*score_samples >= 2"):
        gs.set_estimator("score", "image")
    with pytest.raises(ValueError, match="image.*score_samples >= 2"):
        gs.set_estimator("score", "image", 0.0, samples=1)
    with pytest.raises(ValueError, match="score_baseline"):
        gs.set_estimator("score", "mean", 0.0, samples=2)
    assert gs.estimator == {"kind": "pathwise"}
    gs.set_estimator("score", samples=2)
    assert gs.estimator == {"kind": "score", "baseline": "image", "entropy_weight": 0.0, "samples": 2}, "image is the default above one sample"
    gs.set_estimator("score")
    assert gs.estimator == {"kind": "score", "baseline": "rloo", "entropy_weight": 0.0}
    # the relaxation is needed all the same
    soft, _, _ = _fresh(relax=("gumbel", 1.0, SEED))
    with pytest.raises(ValueError, match="generator_gradient=score.*generator_output="):
        soft.set_estimator("score", samples=2)
    # a kernel set without the entry points, by name
    bare, _, _ = _fresh(K=ScoreRefKernels())
    with pytest.raises(RuntimeError, match="score_samples > 1.*sample_rows_multi, score_advantage_multi, score_rows_multi, score_summary_multi"):
        bare.set_estimator("score", samples=2)
    assert bare.estimator == {"kind": "pathwise"}
    # one image: rloo needs S * B >= 2, which two samples give
    one, _, _ = _fresh(rows=1)
    with pytest.raises(ValueError, match="rloo.*B >= 2"):
        one.set_estimator("score", "rloo")
    one.set_estimator("score", "rloo", 0.0, samples=2)
    one.set_estimator("score", "image", 0.0, samples=2)
    assert one.estimator["baseline"] == "image"


# ---- train.py on the reference kernels --------------------------------------------------------------------------------------------------
@pytest.fixture
def multi_train(cpu_train, monkeypatch):
    """cpu_train with a ScoreMultiRefKernels behind kernels_for."""
    T, _, make = cpu_train
    from sgg_amd import api
    K = ScoreMultiRefKernels()
    monkeypatch.setattr(T, "kernels_for", lambda device: K)
    monkeypatch.setattr(api, "kernels_for", lambda device: K)
    return T, K, make


def _records(tmp, name):
    with open(str(tmp / name / "logs" / "losses.jsonl")) as f:
        return [json.loads(l) for l in f if l.strip()]


def test_parser_rules(multi_train, tmp_path):
    T, K, make = multi_train
    assert T.parse_args([]).score_samples is None
    a = T.parse_args(["--generator_gradient", "score", "--score_samples", "4"])
    assert (a.score_samples, a.score_baseline, a.generator_output, a.relax_hard) == (4, None, "gumbel", True)
    a = T.parse_args(["--generator_gradient", "score", "--score_samples", "16", "--score_baseline", "image"])
    assert (a.score_samples, a.score_baseline) == (16, "image")
    assert T.parse_args(["--generator_gradient", "score", "--score_samples", "1", "--score_baseline", "rloo"]).score_samples == 1
    for bad in (["--score_samples", "2"], ["--generator_gradient", "pathwise", "--score_samples", "2"],
                ["--generator_gradient", "score", "--score_samples", "0"], ["--generator_gradient", "score", "--score_samples", "17"],
                ["--generator_gradient", "score", "--score_samples", "2.5"], ["--generator_gradient", "score", "--score_baseline", "image"],
                ["--generator_gradient", "score", "--score_baseline", "image", "--score_samples", "1"], ["--score_baseline", "image"]):
        with pytest.raises(SystemExit):
            T.parse_args(bad)
    for kw in ({"score_samples": 2}, {"generator_gradient": "score", "score_samples": 0}, {"generator_gradient": "score", "score_samples": 17},
               {"generator_gradient": "score", "score_baseline": "image"}, {"generator_gradient": "score", "score_baseline": "image", "score_samples": 1}):
        with pytest.raises(ValueError):
            make(tmp_path, "bad", resume=False, **kw)
    assert make(tmp_path, "ok", resume=False, generator_gradient="score", score_samples=2).score == \
        {"kind": "score", "baseline": "image", "entropy_weight": 0.0, "samples": 2}
    assert make(tmp_path, "ok", resume=False, generator_gradient="score", score_samples=1).score == \
        {"kind": "score", "baseline": "rloo", "entropy_weight": 0.0}


def test_train_run_with_three_samples_resumes_bit_for_bit_and_records_the_keys(multi_train, tmp_path):
    T, K, make = multi_train
    kw = dict(generator_gradient="score", entropy_weight=0.01, score_samples=3, critic_iters=2)
    gan = make(tmp_path, "whole", resume=False, **kw)
    gan.train(max_iterations=3, log_every=1, validate_every=1, test_at_end=False)
    recs = [r for r in _records(tmp_path, "whole") if "triples_per_s" in r]
    assert len(recs) == 3
    for r in recs:
        sc = r["score"]
        assert sorted(sc) == ["adv_rms", "baseline", "entropy_token", "entropy_weight", "logp_token", "reward", "samples"]
        assert sc["baseline"] == "image" and sc["samples"] == 3 and sc["entropy_weight"] == 0.01
        assert sc["logp_token"] < 0.0 < sc["entropy_token"] <= np.log(11.0) + 1e-12 and sc["adv_rms"] >= 0.0
        assert abs(sc["reward"] + r["gen_loss"]) < 2e-6, "the mean reward is the mean critic score over all samples"
    ck = torch.load(gan._ckpt_path())
    assert ck["generator_output"] == {"mode": "gumbel", "tau": [1.0, 1.0, 0], "hard": True,
                                      "gradient": {"kind": "score", "baseline": "image", "entropy_weight": 0.01, "samples": 3}}
    assert [c for c in K.calls if c in MULTI] == list(MULTI) * 3 and not [c for c in K.calls if c in NEW]
    # the generator update's draw number is the one the single-sample path takes; the critic's updates keep one sample each
    assert [c["draw"] for c in K.multi_log if c["op"] == "sample"] == [T.relax_draw(it, 2, 0, 2, 1) for it in range(3)]
    assert len([c for c in K.hard_log if c["op"] == "fwd" and c["draw"] < 2 ** 63]) == 6
    # stopped after one iteration and resumed WITHOUT the flags: everything comes from the checkpoint, the same weights bit for bit
    part = make(tmp_path, "parts", resume=False, **kw)
    part.train(max_iterations=1, log_every=1, validate_every=1, test_at_end=False)
    rest = make(tmp_path, "parts", resume=True, critic_iters=2)
    rest.train(max_iterations=3, log_every=1, validate_every=1, test_at_end=False)
    assert rest.score == {"kind": "score", "baseline": "image", "entropy_weight": 0.01, "samples": 3}
    ck2 = torch.load(rest._ckpt_path())
    assert ck2["generator_output"] == ck["generator_output"]
    for net in ("G", "D"):
        for name, t in ck[net].items():
            assert torch.equal(t, ck2[net][name]), "%s %s differs after the resume" % (net, name)
    again = make(tmp_path, "parts", resume=True, **kw)
    assert again.load_checkpoint() and again.score == rest.score
    # contradicting flags: before anything is loaded
    for bad in ({"generator_gradient": "score", "score_samples": 4}, {"generator_gradient": "score", "score_samples": 1},
                {"generator_gradient": "score", "score_samples": 3, "score_baseline": "rloo"}, {"generator_gradient": "pathwise"}):
        ev = make(tmp_path, "parts", resume=False, **bad)
        with pytest.raises(ValueError, match="contradicts"):
            ev.load_checkpoint()
        assert ev.itr == 0, "nothing was loaded"


def test_single_sample_checkpoints_keep_their_keys_and_refuse_the_flag(multi_train, tmp_path):
    T, K, make = multi_train
    one = make(tmp_path, "one", resume=False, generator_gradient="score", score_samples=1)
    one.train(max_iterations=1, log_every=1, validate_every=0, test_at_end=False)
    ck = torch.load(one._ckpt_path())
    assert ck["generator_output"]["gradient"] == {"kind": "score", "baseline": "rloo", "entropy_weight": 0.0}
    rec = [r for r in _records(tmp_path, "one") if "triples_per_s" in r]
    assert "samples" not in rec[0]["score"] and not [c for c in K.calls if c in MULTI]
    bad = make(tmp_path, "one", resume=False, generator_gradient="score", score_samples=2)
    with pytest.raises(ValueError, match="--score_samples 2 contradicts"):
        bad.load_checkpoint()
    assert bad.itr == 0
    again = make(tmp_path, "one", resume=False, generator_gradient="score", score_samples=1)
    assert again.load_checkpoint() and "samples" not in again.score


def test_evaluation_of_a_multi_sample_checkpoint_labels_its_output(multi_train, tmp_path):
    T, K, make = multi_train
    gan = make(tmp_path, "score", resume=False, generator_gradient="score", score_samples=2)
    gan.train(max_iterations=2, log_every=1, validate_every=0, test_at_end=False)
    fresh = make(tmp_path, "score", resume=False)          # an evaluation run (--test_only): no flags, everything from the checkpoint
    assert fresh.load_checkpoint() and fresh.score == {"kind": "score", "baseline": "image", "entropy_weight": 0.0, "samples": 2} and fresh.itr == 2
    n = len([c for c in K.calls if c in MULTI])
    label = {"mode": "gumbel", "tau": 1.0, "hard": True, "gradient": "score", "samples": 2}
    out = str(tmp_path / "recalls.txt")
    fresh.test(max_images=1, out_path=out)
    assert "# generator_output: " + json.dumps(label) in open(out).read()
    index = fresh.write_predictions(str(tmp_path / "graphs"), max_images=1)
    assert index["generator_output"] == label and json.load(open(str(tmp_path / "graphs" / "index.json")))["generator_output"] == label
    assert len([c for c in K.calls if c in MULTI]) == n, "evaluation launches nothing of the estimator"
