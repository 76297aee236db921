"""One training step of the decoder in float64: the whole-sequence forward of the reference's CoreDecoder (radae_base.py:291-354, the stateless form train.py:257-263
uses) with every activation the backward pass needs, distortion_loss (radae_base.py:50-68) with its gradient, the backward pass written out by hand, and Adam
(train.py:93-94, :147-150).  It is the model rade_train_* (radae_amd/csrc/rade_train.hip) is held to per tensor (tests/test_train_gpu.py), and is itself held to a torch
restatement, to finite differences and to torch.optim.Adam (tests/test_train_ref_host.py).  numpy only; holds no fixtures.  The layer arithmetic is core_ref.Decoder's
(same gate order, same sigmoid, same concat layout, core_ref.py:8-9), over B sequences at once.

Deviations shared with the device code: the uniform noise of n() is left out and its clamp is the identity (every argument lies in [-1, 1]); the GLU's effective weight
is the parameter (weight_norm_grads of radae_amd/train.py maps its gradient to the reference's (g, v)).

MISTAKES names the faults backward() can be asked to plant; the host test shows that each one exceeds TOL on its own tensor by at least 10 times.
"""
import numpy as np

from core_ref import DEC_W, _sigmoid, column_name

NL, H = 5, 96
GRU_IN = tuple(96 + 128 * l for l in range(NL))         # width of x a GRU reads
CONV_IN = tuple(192 + 128 * l for l in range(NL))       # width of x a conv reads: the GRU's input and its GLU
BETAS, EPS = (0.8, 0.95), 1e-8                           # train.py:147
MISTAKES = ("gate_order", "no_r_factor", "tap0_row", "cross_sequence", "skip_last_step", "overwrite_concat", "sign0_is_1", "output_80")

# name -> shape, in the order of the flat buffers (rade_train_param)
PARAM_TABLE = [("dec_dense1.w", (96, 80)), ("dec_dense1.b", (96,))]
for _l in range(NL):
    PARAM_TABLE += [(f"dec_gru[{_l}].w_ih", (288, GRU_IN[_l])), (f"dec_gru[{_l}].w_hh", (288, 96)), (f"dec_gru[{_l}].b_ih", (288,)), (f"dec_gru[{_l}].b_hh", (288,)),
                    (f"dec_glu[{_l}].w", (96, 96)), (f"dec_conv[{_l}].w", (32, CONV_IN[_l], 2)), (f"dec_conv[{_l}].b", (32,))]
PARAM_TABLE += [("dec_output.w", (84, DEC_W)), ("dec_output.b", (84,))]
N_FLOATS = sum(int(np.prod(s)) for _, s in PARAM_TABLE)

# TOL[tensor class]: the largest max|d| / max|g| a device result may show against this model.  Measured, not chosen: tests/test_train_ref_host.py runs torch's float32
# CPU autograd of the same graph -- a second float32 evaluation in another summation order -- against this model at the GPU test's shapes and weights, and TOL is 4 times
# the largest figure seen, rounded up in the second digit.  The factor 4 covers a different but legitimate summation order, not a mistake: every planted mistake exceeds
# TOL at least 10 times.  Measured max|d| / max|g| of float32 torch on one thread (grad: the worst parameter tensor):
#     weights      (B, T)      grad     dz_hat   loss     features_hat   x
#     random       (3, 5)      5.7e-7   3.7e-7   2.1e-7   1.7e-7         3.2e-7
#     random       (17, 33)    5.7e-7   2.9e-7   9.7e-8   6.8e-7         5.4e-7
#     random       (8, 64)     6.0e-7   3.5e-7   7.0e-8   7.4e-7         5.1e-7
#     model19      (3, 5)      7.6e-7   4.9e-7   5.7e-8   2.9e-7         1.2e-6
#     model19      (17, 33)    2.6e-6   4.1e-6   2.1e-7   3.0e-6         6.3e-6
#     model19      (8, 64)     6.2e-6   6.5e-6   9.6e-8   1.2e-6         3.0e-6
#     random x 2   (3, 5)      5.7e-7   3.6e-7   1.0e-7   2.4e-7         7.6e-7
#     random x 2   (17, 33)    5.7e-7   3.3e-7   1.1e-7   6.3e-7         1.6e-6
#     random x 2   (8, 64)     4.6e-7   3.1e-7   8.7e-8   5.8e-7         1.2e-6
# The host test asserts that float32 torch stays within TOL / 4.
TOL = {"grad": 2.5e-5, "dz_hat": 2.7e-5, "loss": 8.5e-7, "features_hat": 1.3e-5, "x": 2.6e-5}


def tensor_names():
    return [n for n, _ in PARAM_TABLE]


def params_from_model(model, dtype=np.float64):
    """{name: array} of a dnnw.Model's decoder, in PARAM_TABLE's shapes"""
    P = {"dec_dense1.w": model.dec_dense1.w, "dec_dense1.b": model.dec_dense1.b, "dec_output.w": model.dec_output.w, "dec_output.b": model.dec_output.b}
    for l in range(NL):
        g, c = model.dec_gru[l], model.dec_conv[l]
        P.update({f"dec_gru[{l}].w_ih": g.w_ih, f"dec_gru[{l}].w_hh": g.w_hh, f"dec_gru[{l}].b_ih": g.b_ih, f"dec_gru[{l}].b_hh": g.b_hh,
                  f"dec_glu[{l}].w": model.dec_glu[l].w, f"dec_conv[{l}].w": c.w, f"dec_conv[{l}].b": c.b})
    out = {n: np.array(P[n], dtype) for n, _ in PARAM_TABLE}
    for n, s in PARAM_TABLE:
        assert out[n].shape == s, (n, out[n].shape, s)
    return out


def random_params(seed, scale=1.0, dtype=np.float64):
    """a seeded set of the size of a trained one: uniform in +-scale / sqrt(fan in), float32 values"""
    rng = np.random.default_rng(seed)
    out = {}
    for n, s in PARAM_TABLE:
        fan = s[1] * (2 if len(s) == 3 else 1) if len(s) > 1 else 16
        out[n] = (rng.uniform(-1, 1, s) * scale / np.sqrt(fan)).astype(np.float32).astype(dtype)
    return out


def flatten(P, dtype=np.float32):
    return np.concatenate([np.asarray(P[n], dtype).ravel() for n, _ in PARAM_TABLE])


def unflatten(flat):
    out, o = {}, 0
    for n, s in PARAM_TABLE:
        k = int(np.prod(s)); out[n] = np.asarray(flat[o:o + k]).reshape(s); o += k
    return out


# ---- forward --------------------------------------------------------------------------------------------------------------------------------------------------
def forward(P, z_hat):
    """z_hat [B, T, 80] -> saved activations: x [B, T, 736], per layer r, z, n, hn (= W_hn h + b_hn), h [B, T, 96] and the GLU's sigmoid s; out [B, T, 84].
    features_hat [B, 4 T, 21] is out reshaped.  Zero GRU state and zero conv history at the start of every sequence."""
    zin = np.asarray(z_hat, np.float64)
    B, T, _ = zin.shape
    x = np.zeros((B, T, DEC_W))
    x[..., :96] = np.tanh(zin @ P["dec_dense1.w"].T + P["dec_dense1.b"])
    S = {"z_in": zin, "x": x, "layers": []}
    for l in range(NL):
        kg, kc = GRU_IN[l], CONV_IN[l]
        w_ih, w_hh, b_ih, b_hh = (P[f"dec_gru[{l}].{k}"] for k in ("w_ih", "w_hh", "b_ih", "b_hh"))
        gi = x[..., :kg] @ w_ih.T + b_ih
        L = {k: np.zeros((B, T, H)) for k in ("r", "z", "n", "hn", "h")}
        h = np.zeros((B, H))
        for t in range(T):
            gh = h @ w_hh.T + b_hh
            r = _sigmoid(gi[:, t, :H] + gh[:, :H]); zt = _sigmoid(gi[:, t, H:2 * H] + gh[:, H:2 * H])
            n = np.tanh(gi[:, t, 2 * H:] + r * gh[:, 2 * H:])
            h = (h - n) * zt + n
            L["r"][:, t], L["z"][:, t], L["n"][:, t], L["hn"][:, t], L["h"][:, t] = r, zt, n, gh[:, 2 * H:], h
        L["s"] = _sigmoid(L["h"] @ P[f"dec_glu[{l}].w"].T)
        x[..., kg:kc] = L["h"] * L["s"]
        w, xp = P[f"dec_conv[{l}].w"], np.zeros((B, T, kc))
        xp[:, 1:] = x[:, :-1, :kc]                                   # the older tap reads row t - 1, zeros ahead of row 0
        x[..., kc:kc + 32] = np.tanh(xp @ w[:, :, 0].T + x[..., :kc] @ w[:, :, 1].T + P[f"dec_conv[{l}].b"])
        S["layers"].append(L)
    S["out"] = x @ P["dec_output.w"].T + P["dec_output.b"]
    return S


def features_hat(S):
    B, T, _ = S["out"].shape
    return S["out"].reshape(B, 4 * T, 21)


# ---- loss -----------------------------------------------------------------------------------------------------------------------------------------------------
def loss(features, fhat, sign0_is_1=False):
    """distortion_loss(features [B, F, 20 | 21], fhat [B, F, 21]) as written -> (loss_by_batch [B], total = their mean, d total / d fhat [B, F, 21]).  The pitch,
    correlation and data terms broadcast over the 18 cepstral columns before the mean; |.| has gradient sign (0 at 0); the pitch weight takes no gradient."""
    y, p = np.asarray(features, np.float64), np.asarray(fhat, np.float64)
    B, F, nf = y.shape
    assert nf in (20, 21) and p.shape == (B, F, 21)
    ceps = p[..., :18] - y[..., :18]
    pitch = 2 * (p[..., 18:19] - y[..., 18:19])
    corr = p[..., 19:20] - y[..., 19:20]
    pw = np.maximum(y[..., 19:20] + 0.5, 0.0) ** 2
    data = p[..., 20:21] - y[..., 20:21] if nf == 21 else np.zeros_like(corr)
    c1, c2, c3 = 3.0 * (10 / 18), 1 / 18, 0.5 / 18
    per = np.mean(ceps ** 2 + c1 * np.abs(pitch) * pw + c2 * corr ** 2 + c3 * data ** 2, axis=-1)
    by_batch = per.mean(axis=-1)
    G = 1.0 / (B * F * 18)
    sg = np.sign(pitch)
    if sign0_is_1:
        sg = np.where(pitch == 0, 1.0, sg)
    d = np.zeros_like(p)
    d[..., :18] = 2 * ceps * G
    d[..., 18:19] = 18 * c1 * pw * sg * 2 * G
    d[..., 19:20] = 18 * c2 * 2 * corr * G
    d[..., 20:21] = 18 * c3 * 2 * data * G                            # 0 with 20 features
    return by_batch, float(by_batch.mean()), d


# ---- backward -------------------------------------------------------------------------------------------------------------------------------------------------
def backward(P, S, dfhat, mistake=None):
    """d / d z_hat [B, T, 80] and d / d every parameter of sum(dfhat * features_hat), by hand.  BPTT runs from row T - 1 to row 0 of each sequence; the concat
    buffer's gradient accumulates over every layer that read a column; the conv's tap 0 sends gradient to row t - 1 and none out of row 0.
    mistake: one of MISTAKES, planted."""
    assert mistake is None or mistake in MISTAKES
    x = S["x"]
    B, T, _ = x.shape
    dout = np.asarray(dfhat, np.float64).reshape(B, T, 84).copy()
    if mistake == "output_80":
        dout[..., 80:] = 0.0
    G = {}
    flat = lambda a: a.reshape(B * T, -1)
    G["dec_output.w"], G["dec_output.b"] = flat(dout).T @ flat(x), flat(dout).sum(0)
    dx = dout @ P["dec_output.w"]
    for l in reversed(range(NL)):
        kg, kc = GRU_IN[l], CONV_IN[l]
        L = S["layers"][l]

        def add(cols, v, dx=dx):
            if mistake == "overwrite_concat":
                dx[..., :cols] = v
            else:
                dx[..., :cols] += v
        # conv
        w = P[f"dec_conv[{l}].w"]
        dc = dx[..., kc:kc + 32] * (1 - x[..., kc:kc + 32] ** 2)
        xp = np.zeros((B, T, kc)); xp[:, 1:] = x[:, :-1, :kc]
        G[f"dec_conv[{l}].w"] = np.stack([flat(dc).T @ flat(xp), flat(dc).T @ flat(x[..., :kc])], axis=-1)
        G[f"dec_conv[{l}].b"] = flat(dc).sum(0)
        add(kc, dc @ w[:, :, 1])
        d0 = dc @ w[:, :, 0]
        if mistake == "tap0_row":
            dx[..., :kc] += d0
        elif mistake == "cross_sequence":                              # rows in one run b T + t: row 0 of sequence b + 1 sends into the last row of sequence b
            f = dx.reshape(B * T, -1); f[:-1, :kc] += d0.reshape(B * T, -1)[1:]
        else:
            dx[:, :-1, :kc] += d0[:, 1:]
        # GLU: g = h s, s = sigmoid(W h)
        wg = P[f"dec_glu[{l}].w"]
        dg = dx[..., kg:kc]
        da = dg * L["h"] * L["s"] * (1 - L["s"])
        G[f"dec_glu[{l}].w"] = flat(da).T @ flat(L["h"])
        dh_ext = dg * L["s"] + da @ wg
        # GRU, back through time
        w_ih, w_hh = P[f"dec_gru[{l}].w_ih"], P[f"dec_gru[{l}].w_hh"]
        dgi, dgh = np.zeros((B, T, 3 * H)), np.zeros((B, T, 3 * H))
        carry = np.zeros((B, H))
        for t in reversed(range(T)):
            if mistake == "skip_last_step" and t == T - 1 and T > 1:
                continue
            hp = L["h"][:, t - 1] if t else np.zeros((B, H))
            r, zt, n, hn = L["r"][:, t], L["z"][:, t], L["n"][:, t], L["hn"][:, t]
            dh = dh_ext[:, t] + carry
            dnt = dh * (1 - zt) * (1 - n * n)
            dzt = dh * (hp - n) * zt * (1 - zt)
            drt = dnt * hn * r * (1 - r)
            if mistake == "gate_order":
                drt, dzt = dzt, drt
            dgi[:, t] = np.concatenate([drt, dzt, dnt], -1)
            dgh[:, t] = np.concatenate([drt, dzt, dnt if mistake == "no_r_factor" else dnt * r], -1)
            carry = dh * zt + dgh[:, t] @ w_hh
        hprev = np.zeros((B, T, H)); hprev[:, 1:] = L["h"][:, :-1]
        G[f"dec_gru[{l}].w_ih"], G[f"dec_gru[{l}].b_ih"] = flat(dgi).T @ flat(x[..., :kg]), flat(dgi).sum(0)
        G[f"dec_gru[{l}].w_hh"], G[f"dec_gru[{l}].b_hh"] = flat(dgh).T @ flat(hprev), flat(dgh).sum(0)
        add(kg, dgi @ w_ih)
    dd = dx[..., :96] * (1 - x[..., :96] ** 2)
    G["dec_dense1.w"], G["dec_dense1.b"] = flat(dd).T @ flat(S["z_in"]), flat(dd).sum(0)
    return G, dd @ P["dec_dense1.w"]


def step_grads(P, z_hat, features, mistake=None):
    """forward, loss and backward in one: (saved, loss_by_batch, total, dfhat, grads, dz_hat)"""
    S = forward(P, z_hat)
    by, total, d = loss(features, features_hat(S), sign0_is_1=(mistake == "sign0_is_1"))
    G, dz = backward(P, S, d, None if mistake == "sign0_is_1" else mistake)
    return S, by, total, d, G, dz


# ---- Adam -----------------------------------------------------------------------------------------------------------------------------------------------------
def lr_at(lr, decay, step):
    """train.py:148-150: LambdaLR with 1 / (1 + decay x), x the number of scheduler steps taken"""
    return lr / (1.0 + decay * step)


def adam(p, g, m, v, lr_t, step, betas=BETAS, eps=EPS):
    """torch.optim.Adam (no weight decay, no amsgrad), step counted from 1: returns the new (p, m, v)"""
    b1, b2 = betas
    m = m + (1 - b1) * (g - m)
    v = b2 * v + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    return p - (lr_t / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + eps), m, v


class UpdateBound:
    """How far a float32 Adam update of one tensor may stand from this model's, step by step, given that each step's gradient was within dg of the model's (the
    caller checks that with check_grads first, so the drift of the parameters is inside dg).  Carried: dm, dv, the bounds on |m - model m| and |v - model v|:
        m' = 0.8 m + 0.2 g          dm' = 0.8 dm + 0.2 dg + 4 u (|m| + |g|)                          (u = 2^-24: the kernel's roundings, rade_train.hip's header)
        v' = 0.95 v + 0.05 g^2      dv' = 0.95 dv + 0.05 (2 |g| dg + dg^2) + 5 u (v + g^2)
        |sqrt v'_dev - sqrt v'| <= dr = min(sqrt dv', dv' / sqrt v'),   D = sqrt v' / sqrt bc2 + eps,   D_lo = max(D - dr / sqrt bc2, eps)
        |update_dev - update| <= s (dm' / D_lo + |m'| (dr / sqrt bc2) / (D D_lo)) + 8 u |update| + u |p|,   s = lr / bc1.
    Nothing is masked: where v' is as small as its own error -- the first step's sign of a gradient that float32 does not fix -- the bound itself grows to the update's size."""

    def __init__(self, shape):
        self.dm, self.dv = np.zeros(shape), np.zeros(shape)

    def step(self, p, g, m, v, lr_t, step, dg, betas=BETAS, eps=EPS):
        """p, m, v: the model's values ahead of the step; returns (the model's new (p, m, v), the bound on the update's difference per element)"""
        u = 2.0 ** -24
        b1, b2 = betas
        pn, mn, vn = adam(p, g, m, v, lr_t, step, betas, eps)
        self.dm = b1 * self.dm + (1 - b1) * dg + 4 * u * (np.abs(m) + np.abs(g))
        self.dv = b2 * self.dv + (1 - b2) * (2 * np.abs(g) * dg + dg * dg) + 5 * u * (v + g * g)
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        r = np.sqrt(vn)
        with np.errstate(divide="ignore", invalid="ignore"):
            dr = np.minimum(np.sqrt(self.dv), np.where(r > 0, self.dv / r, np.inf))
        D = r / np.sqrt(bc2) + eps
        D_lo = np.maximum(D - dr / np.sqrt(bc2), eps)
        s = lr_t / bc1
        upd = pn - p
        return (pn, mn, vn), s * (self.dm / D_lo + np.abs(mn) * (dr / np.sqrt(bc2)) / (D * D_lo)) + 8 * u * np.abs(upd) + u * np.abs(p)


# ---- comparison -----------------------------------------------------------------------------------------------------------------------------------------------
def layer_of(name, index):
    """the layer an element of a tensor belongs to, for a message"""
    if name in ("x", "dx"):
        return column_name(int(index[-1]))
    if name in ("features_hat", "dfhat"):
        return f"output column {int(index[-1])}"
    if name == "dz_hat":
        return f"latent {int(index[-1])}"
    return name.split(".")[0]


def rel_errors(got, want):
    """(max|d| / max|g|, ||d||_2 / ||g||_2, index of the worst element); a tensor that is all zero compares absolutely"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    d = got - want
    if not np.isfinite(d).all():
        return np.inf, np.inf, np.unravel_index(int(np.argmax(~np.isfinite(d))), d.shape)
    sm, s2 = np.abs(want).max(), np.sqrt((want ** 2).sum())
    return float(np.abs(d).max() / (sm if sm > 0 else 1.0)), float(np.sqrt((d ** 2).sum()) / (s2 if s2 > 0 else 1.0)), np.unravel_index(int(np.argmax(np.abs(d))), d.shape)


def check_tensor(name, got, want, tol, what=""):
    """max|d| / max|g| <= tol, or an AssertionError that names the tensor, the element and the element's layer; returns the two figures"""
    e_max, e_2, idx = rel_errors(got, want)
    if not e_max <= tol:
        g, w = np.asarray(got, np.float64)[idx], np.asarray(want, np.float64)[idx]
        raise AssertionError(f"{what}{name}{list(map(int, idx))} ({layer_of(name, idx)}): got {g!r}, float64 model {w!r}; max|d| / max|g| = {e_max:.3e} > {tol:.1e}, "
                             f"||d|| / ||g|| = {e_2:.3e}")
    return e_max, e_2


def check_grads(got, want, dz_got, dz_want, tol=None, what=""):
    """every parameter tensor and dz_hat; returns {name: (max figure, 2-norm figure)}"""
    out = {n: check_tensor(n, got[n], want[n], TOL["grad"] if tol is None else tol, what) for n, _ in PARAM_TABLE}
    out["dz_hat"] = check_tensor("dz_hat", dz_got, dz_want, TOL["dz_hat"] if tol is None else tol, what)
    return out


# ---- the reference live (a child process of tests/test_train_ref_host.py: `python train_ref.py REFERENCE_DIR`) ------------------------------------------------------
def _live(ref):
    """CoreDecoder of the reference itself in double, n() patched to its clamp, distortion_loss(...).mean().backward(): every gradient, dz and the loss against this
    model at (B, T) = (3, 5) and (17, 33), to 1e-10 relative.  The GLU's weight goes through weight_norm_grads."""
    import os
    import sys
    import torch
    sys.path.insert(0, os.path.join(ref, "radae"))
    import radae_base
    from radae_amd.train import weight_norm_grads
    torch.set_default_dtype(torch.float64)
    radae_base.n = lambda x: torch.clamp(x, min=-1.0, max=1.0)
    torch.manual_seed(11)
    dec = radae_base.CoreDecoder(80, 21)
    sd = dict(dec.named_parameters())
    eff = {l: getattr(dec, f"glu{l + 1}").gate.weight.detach().numpy().copy() for l in range(NL)}
    P = {"dec_dense1.w": sd["dense_1.weight"], "dec_dense1.b": sd["dense_1.bias"], "dec_output.w": sd["output.weight"], "dec_output.b": sd["output.bias"]}
    for l in range(NL):
        P.update({f"dec_gru[{l}].w_ih": sd[f"gru{l + 1}.weight_ih_l0"], f"dec_gru[{l}].w_hh": sd[f"gru{l + 1}.weight_hh_l0"], f"dec_gru[{l}].b_ih": sd[f"gru{l + 1}.bias_ih_l0"],
                  f"dec_gru[{l}].b_hh": sd[f"gru{l + 1}.bias_hh_l0"], f"dec_conv[{l}].w": sd[f"conv{l + 1}.conv.weight"], f"dec_conv[{l}].b": sd[f"conv{l + 1}.conv.bias"]})
    Pn = {k: v.detach().numpy().copy() for k, v in P.items()}
    Pn.update({f"dec_glu[{l}].w": eff[l] for l in range(NL)})
    rng = np.random.default_rng(5)
    for nf in (21, 20):
        for B, T in ((3, 5), (17, 33)):
            z = torch.tensor(rng.standard_normal((B, T, 80)), requires_grad=True)
            y = torch.tensor(rng.standard_normal((B, 4 * T, nf)))
            dec.zero_grad()
            by = radae_base.distortion_loss(y, dec(z))
            by.mean().backward()
            _, by64, total, _, G, dz = step_grads(Pn, z.detach().numpy(), y.numpy())
            check_tensor("loss", by64, by.detach().numpy(), 1e-10, f"live ({B}, {T}, {nf}): ")
            check_tensor("dz_hat", dz, z.grad.numpy(), 1e-10, f"live ({B}, {T}, {nf}): ")
            for k, v in P.items():
                check_tensor(k, G[k], v.grad.numpy(), 1e-10, f"live ({B}, {T}, {nf}): ")
            for l in range(NL):
                par = getattr(dec, f"glu{l + 1}").gate.parametrizations.weight
                dg, dv = weight_norm_grads(G[f"dec_glu[{l}].w"], par.original0.detach().numpy(), par.original1.detach().numpy())
                check_tensor(f"dec_glu[{l}].w", dg, par.original0.grad.numpy(), 1e-10, f"live g ({B}, {T}, {nf}): ")
                check_tensor(f"dec_glu[{l}].w", dv, par.original1.grad.numpy(), 1e-10, f"live v ({B}, {T}, {nf}): ")
    print("live ok")


if __name__ == "__main__":
    import sys
    _live(sys.argv[1])
