"""Host tests (no GPU) of the float64 model of the decoder's training step (tests/train_ref.py), the model tests/test_train_gpu.py holds rade_train_* to: against the
reference live, against a torch restatement written here (autograd in double), against central differences, Adam against torch.optim.Adam and the learning-rate
schedule against LambdaLR; the planted mistakes against TOL; and TOL itself against a float32 evaluation of the same graph."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import train_ref as tr

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = ((3, 5), (17, 33))


# ---- a torch restatement of the graph (radae_base.py:333-354 with n() = the identity, nn.GRU's cell written out, MyConv as two products) ----------------------------
def torch_forward(P, z):
    B, T, _ = z.shape
    x = torch.tanh(z @ P["dec_dense1.w"].T + P["dec_dense1.b"])
    for l in range(tr.NL):
        gi = x @ P[f"dec_gru[{l}].w_ih"].T + P[f"dec_gru[{l}].b_ih"]
        w_hh, b_hh = P[f"dec_gru[{l}].w_hh"], P[f"dec_gru[{l}].b_hh"]
        h, hs = torch.zeros(B, 96, dtype=z.dtype), []
        for t in range(T):
            gh = h @ w_hh.T + b_hh
            r = torch.sigmoid(gi[:, t, :96] + gh[:, :96]); u = torch.sigmoid(gi[:, t, 96:192] + gh[:, 96:192])
            n = torch.tanh(gi[:, t, 192:] + r * gh[:, 192:])
            h = (1 - u) * n + u * h
            hs.append(h)
        hh = torch.stack(hs, 1)
        x = torch.cat([x, hh * torch.sigmoid(hh @ P[f"dec_glu[{l}].w"].T)], -1)
        xp = torch.cat([torch.zeros_like(x[:, :1]), x[:, :-1]], 1)
        w = P[f"dec_conv[{l}].w"]
        x = torch.cat([x, torch.tanh(xp @ w[:, :, 0].T + x @ w[:, :, 1].T + P[f"dec_conv[{l}].b"])], -1)
    out = x @ P["dec_output.w"].T + P["dec_output.b"]
    return out.reshape(B, 4 * T, 21), x


def torch_loss(y, p):
    """distortion_loss (radae_base.py:50-68) -> loss_by_batch"""
    ceps = p[..., :18] - y[..., :18]
    pitch = 2 * (p[..., 18:19] - y[..., 18:19])
    corr = p[..., 19:20] - y[..., 19:20]
    pw = torch.relu(y[..., 19:20] + 0.5) ** 2
    data = p[..., 20:21] - y[..., 20:21] if y.shape[-1] == 21 else 0
    return torch.mean(ceps ** 2 + 3. * (10 / 18) * torch.abs(pitch) * pw + (1 / 18) * corr ** 2 + (0.5 / 18) * data ** 2, dim=-1).mean(dim=-1)


def torch_step(P64, z, y, dtype):
    """(loss_by_batch, features_hat, x, grads, dz) of torch autograd in dtype, as float64 numpy"""
    P = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in P64.items()}
    zt = torch.tensor(z, dtype=dtype, requires_grad=True)
    fh, x = torch_forward(P, zt)
    by = torch_loss(torch.tensor(y, dtype=dtype), fh)
    by.mean().backward()
    f = lambda t: t.detach().double().numpy()
    return f(by), f(fh), f(x), {k: f(v.grad) for k, v in P.items()}, f(zt.grad)


def inputs(B, T, nf=21, seed=0):
    """float32 values, as the device gets them"""
    rng = np.random.default_rng(1000 * B + T + seed)
    return rng.standard_normal((B, T, 80)).astype(np.float32).astype(np.float64), rng.standard_normal((B, 4 * T, nf)).astype(np.float32).astype(np.float64)


def model19():
    from radae_amd import abi, dnnw
    return tr.params_from_model(dnnw.load_model(abi.DEFAULT_BLOB))


@pytest.fixture(scope="module")
def weight_sets():
    return {"random": tr.random_params(1), "model19": model19(), "random x 2": tr.random_params(1, scale=2.0)}


@pytest.fixture(scope="module")
def model_steps(weight_sets):
    """the float64 model's step at every (weights, shape) the tests below share, computed once"""
    made = {}

    def get(name, B, T, nf=21):
        if (name, B, T, nf) not in made:
            z, y = inputs(B, T, nf)
            made[name, B, T, nf] = (z, y) + tr.step_grads(weight_sets[name], z, y)
        return made[name, B, T, nf]
    return get


def test_the_model_against_the_reference_live():
    ref = os.environ.get("RADAE_REFERENCE") or "/root/reference"
    if not os.path.isfile(os.path.join(ref, "radae", "radae_base.py")):
        pytest.skip("the reference is not on this machine")
    r = subprocess.run([sys.executable, os.path.join(HERE, "train_ref.py"), ref], capture_output=True, text=True,
                       env={**os.environ, "PYTHONPATH": HERE + os.pathsep + os.path.dirname(HERE)})
    assert r.returncode == 0 and r.stdout.strip().endswith("live ok"), r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("B, T", SHAPES)
@pytest.mark.parametrize("nf", (21, 20))
def test_the_model_against_torch_autograd_in_double(model_steps, weight_sets, B, T, nf):
    z, y, S, by, total, d, G, dz = model_steps("random", B, T, nf)
    tby, tfh, tx, tG, tdz = torch_step(weight_sets["random"], z, y, torch.float64)
    tr.check_tensor("loss", by, tby, 1e-10)
    tr.check_tensor("features_hat", tr.features_hat(S), tfh, 1e-10)
    tr.check_tensor("x", S["x"], tx, 1e-10)
    tr.check_grads(G, tG, dz, tdz, tol=1e-10)


def test_the_model_against_central_differences(weight_sets):
    """a handful of weights of every tensor, and of z_hat: (L(w + e) - L(w - e)) / 2e in double"""
    P = weight_sets["random"]
    z, y = inputs(3, 5)
    _, _, _, _, G, dz = tr.step_grads(P, z, y)
    rng = np.random.default_rng(9)

    def total(Pq, zq):
        return tr.loss(y, tr.features_hat(tr.forward(Pq, zq)))[1]
    e = 1e-6
    for name, shape in tr.PARAM_TABLE + [("dz_hat", z.shape)]:
        for _ in range(3):
            idx = tuple(int(rng.integers(s)) for s in shape)
            vals = []
            for sgn in (1, -1):
                Pq, zq = {k: v.copy() for k, v in P.items()}, z.copy()
                (zq if name == "dz_hat" else Pq[name])[idx] += sgn * e
                vals.append(total(Pq, zq))
            fd, g = (vals[0] - vals[1]) / (2 * e), (dz if name == "dz_hat" else G[name])[idx]
            scale = np.abs(dz if name == "dz_hat" else G[name]).max()
            assert abs(fd - g) <= 1e-6 * scale + 1e-9, (name, idx, fd, g)


# ---- TOL --------------------------------------------------------------------------------------------------------------------------------------------------------
TOL_CASES = [(w, B, T) for w in ("random", "model19", "random x 2") for B, T in ((3, 5), (17, 33), (8, 64))]


@pytest.fixture(scope="module")
def float32_figures(model_steps, weight_sets):
    """max|d| / max|g| of torch's float32 CPU autograd against the model, per tensor class and case.  One thread: the summation order of torch's products, and
    with it the last digits of these figures, would otherwise follow the number of cores."""
    out, threads = {}, torch.get_num_threads()
    torch.set_num_threads(1)
    for name, B, T in TOL_CASES:
        z, y, S, by, total, d, G, dz = model_steps(name, B, T)
        tby, tfh, tx, tG, tdz = torch_step(weight_sets[name], z, y, torch.float32)
        out[name, B, T] = {"grad": max(tr.rel_errors(tG[k], G[k])[0] for k in G), "dz_hat": tr.rel_errors(tdz, dz)[0], "loss": tr.rel_errors(tby, by)[0],
                           "features_hat": tr.rel_errors(tfh, tr.features_hat(S))[0], "x": tr.rel_errors(tx, S["x"])[0]}
    torch.set_num_threads(threads)
    return out


def test_tol_is_four_times_what_float32_torch_shows(float32_figures):
    """TOL is measured: a second float32 evaluation in another summation order stays within TOL / 4, and TOL is 4 times what it shows at worst, rounded up in the second digit (so at most a tenth more)"""
    for case, fig in float32_figures.items():
        print(case, {k: f"{v:.2e}" for k, v in fig.items()})
    for k, tol in tr.TOL.items():
        worst = max(fig[k] for fig in float32_figures.values())
        assert worst <= tol / 4, (k, worst, tol)
        assert tol <= 4.4 * worst, f"TOL[{k}] = {tol:.1e} is loose: float32 torch shows {worst:.2e} at worst"


OWN_TENSOR = {"gate_order": "dec_gru[4].w_ih", "no_r_factor": "dec_gru[4].w_hh", "tap0_row": "dz_hat", "cross_sequence": "dz_hat", "skip_last_step": "dec_gru[4].w_hh",
              "overwrite_concat": "dz_hat", "sign0_is_1": "dec_output.b", "output_80": "dec_output.w"}


@pytest.mark.parametrize("mistake", tr.MISTAKES)
@pytest.mark.parametrize("B, T", SHAPES)
def test_a_planted_mistake_exceeds_tol_tenfold(model_steps, weight_sets, mistake, B, T):
    P = weight_sets["random"]
    z, y, S, by, total, d, G, dz = model_steps("random", B, T)
    if mistake == "sign0_is_1":                                      # a pitch error that is exactly 0 in every fourth frame
        y = y.copy(); y[:, ::4, 18] = tr.features_hat(S)[:, ::4, 18]
        _, _, _, _, G, dz = tr.step_grads(P, z, y)
    _, _, _, _, Gm, dzm = tr.step_grads(P, z, y, mistake)
    name = OWN_TENSOR[mistake]
    got, want = (dzm, dz) if name == "dz_hat" else (Gm[name], G[name])
    e = tr.rel_errors(got, want)[0]
    tol = tr.TOL["dz_hat" if name == "dz_hat" else "grad"]
    assert e >= 10 * tol, f"{mistake}: {name} moves by {e:.2e} of its largest element, under 10 x TOL = {10 * tol:.1e}"


# ---- Adam and the schedule --------------------------------------------------------------------------------------------------------------------------------------
def test_adam_against_torch_in_double_over_five_steps():
    rng = np.random.default_rng(4)
    p0 = rng.standard_normal(1000)
    pt = torch.tensor(p0.copy(), dtype=torch.float64, requires_grad=True)
    lr, decay = 3e-4, 2.5e-5
    opt = torch.optim.Adam([pt], lr=lr, betas=tr.BETAS, eps=tr.EPS)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda x: 1 / (1 + decay * x))            # train.py:148-150
    p, m, v = p0.copy(), np.zeros(1000), np.zeros(1000)
    for k in range(5):
        g = rng.standard_normal(1000) * 10.0 ** rng.integers(-6, 2, 1000)
        g[:10] = 0.0                                                # v = 0 and g = 0 stay finite
        assert abs(sched.get_last_lr()[0] - tr.lr_at(lr, decay, k)) <= 1e-18
        pt.grad = torch.tensor(g)
        opt.step(); sched.step()
        p, m, v = tr.adam(p, g, m, v, tr.lr_at(lr, decay, k), k + 1)
        assert np.isfinite(p).all() and np.abs(p - pt.detach().numpy()).max() <= 1e-13 * np.abs(p).max()
    assert np.array_equal(p[:10], p0[:10])


def test_weight_norm_grads_against_torch():
    from radae_amd.train import weight_norm_grads
    rng = np.random.default_rng(6)
    g, v, dW = torch.tensor(rng.standard_normal((96, 1)), requires_grad=True), torch.tensor(rng.standard_normal((96, 96)), requires_grad=True), rng.standard_normal((96, 96))
    ((g * v / v.norm(dim=1, keepdim=True)) * torch.tensor(dW)).sum().backward()
    dg, dv = weight_norm_grads(dW, g.detach().numpy(), v.detach().numpy())
    assert np.abs(dg - g.grad.numpy()).max() < 1e-12 and np.abs(dv - v.grad.numpy()).max() < 1e-12
