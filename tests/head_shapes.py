"""Every GEMM and attention launch of both recurrent heads in one G+D step (critic update + generator update), as a function of
(B, L, V): the forward, backward and gradient-penalty (dual-number) passes of sgg_amd/head.py as sgg_amd/step.py drives them.

A launch is a tuple
    ("gemm", mode, M, N, K)              mode 0 = NN (gemm_nn), 1 = NT (gemm_nt), 2 = TN (gemm_tn): the scalars of sgg_gemm_skinny_*
    ("attn_fwd", R, B, L, C, dual)       the scalars of sgg_attn_step_fwd
    ("attn_bwd", R, B, L, C, dual)       the scalars of sgg_attn_step_bwd
`step_launches` returns the set of the launches that go through HipKernels._gemm / attn_step_fwd / attn_step_bwd (what a recording
kernel set sees); `ctx_launches` the three attention-context products, which reach the same GEMM dispatch through
sgg_attn_ctx_gemm_* (head.py:138, 284-296).  tests/test_head_routes_gpu.py compares step_launches with a recorded step."""
C, H, E, T = 512, 512, 300, 3            # params.FEAT_C, NUM_UNITS, EMBED_DIM, T_STEPS


def _forward(out, kind, B, L, V, np_, R, label_rows=None):
    """Head.forward (head.py:142-175)."""
    ind = C + (H if kind == "G" else E)
    width, vout = ind + H, (V if kind == "G" else 1)
    if kind == "D":                                               # the embedding products u_t @ W (head.py:156-164)
        for pl in range(np_):
            if label_rows is not None and pl == 0:
                lo, hi = label_rows
                for a, b in ((0, lo), (hi, R)):                   # head.py:159-161 (the label rows themselves are a row gather)
                    if b > a:
                        out.add(("gemm", 0, b - a, E, V))
            else:
                out.add(("gemm", 0, R, E, V))                     # head.py:164
    out.add(("gemm", 0, np_ * R, L, H))                           # head.py:167  c_t @ W_c
    out.add(("attn_fwd", R, B, L, C, np_ == 2))                   # head.py:168
    out.add(("gemm", 0, np_ * R, 4 * H, width))                   # head.py:169  [z, u, h] @ kernel
    out.add(("gemm", 0, R, vout, H))                              # head.py:172, 174  decoder (per plane)


def _backward(out, kind, B, L, V, np_, R, R_w, labels=False, param_grads=True):
    """Head.backward (head.py:189-259) and its data-only form (head.py:261-276: every row in the dP / dctx rows)."""
    ind = C + (H if kind == "G" else E)
    width, vout = ind + H, (V if kind == "G" else 1)
    if not param_grads:
        R_w = R
    if R_w and param_grads:
        out.add(("gemm", 2, H, vout, R_w))                        # head.py:215  decoder filter gradient (_wgrad, head.py:184-187)
    out.add(("gemm", 1, R, H, vout))                              # head.py:223  decoder dgrad, per plane
    out.add(("gemm", 1, np_ * R, width, 4 * H))                   # head.py:226  gates dgrad
    if R_w:
        out.add(("attn_bwd", R_w, B, L, C, np_ == 2))             # head.py:229
    if R_w < R:
        out.add(("attn_bwd", R - R_w, B, L, C, np_ == 2))         # head.py:231
    out.add(("gemm", 1, np_ * R, H, L))                           # head.py:232  score dgrad
    if R_w and param_grads:
        out.add(("gemm", 2, width, 4 * H, R_w))                   # head.py:236
        if kind == "D":
            if labels and np_ == 1:
                lo, hi = labels
                for a, b in ((0, lo), (hi, R_w)):                 # head.py:241-243
                    if b > a:
                        out.add(("gemm", 2, V, E, b - a))
            else:
                out.add(("gemm", 2, V, E, R_w))                   # head.py:246
        out.add(("gemm", 2, H, L, R_w))                           # head.py:247


def step_launches(B, L, V):
    """The set of _gemm / attn_step launches of GanStep.critic_step followed by GanStep.generator_step."""
    out = set()
    # critic update (step.py:511-547)
    _forward(out, "G", B, L, V, 1, B)                             # G's fakes, forward only
    _forward(out, "D", B, L, V, 1, 3 * B, label_rows=(B, 2 * B))  # fake | real | interpolated rows
    _backward(out, "D", B, L, V, 1, 3 * B, 2 * B, labels=(B, 2 * B))
    _forward(out, "D", B, L, V, 2, B)                             # gradient penalty: dual numbers on the interpolated rows
    _backward(out, "D", B, L, V, 2, B, B)
    out.add(("gemm", 1, B, V, E))                                 # step.py:535  the slopes: cotangent of the interpolated triples
    # generator update (step.py:611-625)
    _forward(out, "G", B, L, V, 1, B)
    _forward(out, "D", B, L, V, 1, B)
    _backward(out, "D", B, L, V, 1, B, 0)
    out.add(("gemm", 1, B, V, E))                                 # step.py:620  the critic's gradient with respect to G's logits
    _backward(out, "G", B, L, V, 1, B, B)
    return out


def ctx_launches(B, L):
    """The attention-context products (sgg_attn_ctx_gemm_fwd / _dgrad / _wgrad, csrc/gemm.hip) of head.py:138, 296, 292."""
    return {("gemm", 0, B, L, L * C), ("gemm", 1, B, L * C, L), ("gemm", 2, L * C, L, B)}


def all_launches(B, L, V):
    return step_launches(B, L, V) | ctx_launches(B, L)


def feature_locations(S):
    """L of an S x S image (params.param_shapes)."""
    import sgg_amd  # noqa: F401
    from sgg_amd.params import feature_side
    return feature_side(S) ** 2
