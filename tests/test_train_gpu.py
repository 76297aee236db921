"""The decoder's training step on the device (rade_train_*, include/rade_batch.h; radae_amd/train.py) against the float64 model of tests/train_ref.py: forward with the
saved concat buffer, the loss and its gradient, every parameter gradient and dz_hat within train_ref.TOL, independence of the sequences of a batch, determinism, the
buffer contract and the refused calls, Adam per element, ten steps on one batch, and the autograd wrapper.

Recorded on the MI355X (max|d| / max|g| against the model, worst case of each class, and train_ref.TOL): parameter gradients 1.3e-6 (dec_conv[2].b, model19 at (17, 33)) of
2.5e-5; dz_hat 1.2e-6 of 2.7e-5; features_hat 1.3e-6 of 1.3e-5; x 4.3e-6 of 2.6e-5; Adam's largest |d p| / bound 0.996; the first three losses of the ten-step run within 0.002 of
their bound; the int8 quantisation of the trained blob moves the output by 0.40 / 0.47 (full scale 6), and the device's two decoders differ by exactly that."""
import numpy as np
import pytest

import core_ref
import train_ref as tr
from bands import Band
from gpu_kit import Dev, stream, sync, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def model_with(P):
    """model19 with the decoder replaced by the parameter set P"""
    import copy
    from radae_amd import abi, dnnw
    m = copy.copy(dnnw.load_model(abi.DEFAULT_BLOB))
    f = lambda a: np.ascontiguousarray(a, np.float32)
    m.dec_dense1, m.dec_output = dnnw.Dense(f(P["dec_dense1.w"]), f(P["dec_dense1.b"])), dnnw.Dense(f(P["dec_output.w"]), f(P["dec_output.b"]))
    m.dec_gru = [dnnw.GRU(*(f(P[f"dec_gru[{l}].{k}"]) for k in ("w_ih", "w_hh", "b_ih", "b_hh"))) for l in range(5)]
    m.dec_glu = [dnnw.Dense(f(P[f"dec_glu[{l}].w"]), np.zeros(96, np.float32)) for l in range(5)]
    m.dec_conv = [dnnw.Conv(f(P[f"dec_conv[{l}].w"]), f(P[f"dec_conv[{l}].b"]), 1) for l in range(5)]
    return m


def inputs(B, T, nf=21, seed=0):
    rng = np.random.default_rng(1000 * B + T + seed)
    return rng.standard_normal((B, T, 80)).astype(np.float32), rng.standard_normal((B, 4 * T, nf)).astype(np.float32)


@pytest.fixture(scope="module")
def weights():
    from radae_amd import abi, dnnw
    return {"model19": tr.params_from_model(dnnw.load_model(abi.DEFAULT_BLOB)), "random": tr.random_params(1)}


@pytest.fixture(scope="module")
def trainers(torch_dev, weights):
    """one DecoderTrainer per (weights, n_features) at the capacity (17, 33), closed when the module ends"""
    from radae_amd.train import DecoderTrainer
    made = {}

    def get(name, nf=21, B=17, T=33):
        if (name, nf, B, T) not in made:
            made[name, nf, B, T] = DecoderTrainer(model_with(weights[name]), B=B, T=T, n_features=nf)
        return made[name, nf, B, T]
    yield get
    for t in made.values():
        t.close()


@pytest.fixture(scope="module")
def model_steps(weights):
    """the float64 model's step, computed once per case"""
    made = {}

    def get(name, B, T, nf=21):
        if (name, B, T, nf) not in made:
            z, y = inputs(B, T, nf)
            made[name, B, T, nf] = (z, y) + tr.step_grads(weights[name], z, y)
        return made[name, B, T, nf]
    return get


def t_(a, dev):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device=dev)


def host_grads(trainer):
    return {k: v.cpu().numpy() for k, v in trainer.grads.items()}


# ---- forward ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("model19", "random"))
@pytest.mark.parametrize("B, T", ((1, 1), (3, 5), (17, 33)))
def test_forward_and_the_saved_concat_buffer(torch_dev, trainers, weights, name, B, T):
    """row counts 1, 15 and 561: no tile edge divides them; B = 17 crosses the 16-sequence scan tile; T = 1 has no recurrence and no conv neighbour"""
    z, _ = inputs(B, T)
    S = tr.forward(weights[name], z)
    t = trainers(name)
    fh = t.forward(t_(z, torch_dev)).cpu().numpy()
    x = t.saved_x().cpu().numpy()
    e = tr.check_tensor("features_hat", fh, tr.features_hat(S), tr.TOL["features_hat"], f"{name} ({B}, {T}): ")
    ex = tr.check_tensor("x", x, S["x"], tr.TOL["x"], f"{name} ({B}, {T}): ")
    print(f"{name} ({B}, {T}): features_hat {e[0]:.2e} of {tr.TOL['features_hat']:.1e}, x {ex[0]:.2e} of {tr.TOL['x']:.1e}")


# ---- loss and gradients -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("model19", "random"))
@pytest.mark.parametrize("nf", (21, 20))
@pytest.mark.parametrize("B, T", ((3, 5), (17, 33)))
def test_every_gradient_within_tol(torch_dev, trainers, model_steps, name, nf, B, T):
    z, y, S, by, total, d, G, dz = model_steps(name, B, T, nf)
    t = trainers(name, nf)
    t.forward(t_(z, torch_dev))
    tot = t.loss(t_(y, torch_dev))
    dz_dev = t.backward()
    what = f"{name} ({B}, {T}, {nf}): "
    tr.check_tensor("loss", t.loss_by_batch.cpu().numpy(), by, tr.TOL["loss"], what)
    assert abs(float(tot) - total) <= tr.TOL["loss"] * abs(total), (float(tot), total)
    tr.check_tensor("dfhat", t.dfeatures_hat.cpu().numpy(), d, tr.TOL["features_hat"], what)
    fig = tr.check_grads(host_grads(t), G, dz_dev.cpu().numpy(), dz, what=what)
    worst = max(fig, key=lambda k: fig[k][0])
    print(f"{what}worst tensor {worst}: max {fig[worst][0]:.2e}, 2-norm {fig[worst][1]:.2e}; dz_hat {fig['dz_hat'][0]:.2e}")


@pytest.mark.parametrize("case", ("pitch_error_0", "pitch_weight_0"))
def test_the_pitch_terms_edge_cases(torch_dev, trainers, weights, case):
    """a pitch error that is exactly 0 in every fourth frame (sign(0) = 0: no gradient from the pitch term there), and features[..., 19] < -0.5 in every third frame
    (the pitch weight is 0).  The device's own features_hat is the loss's input here, so that the zero is a zero on both sides."""
    B, T = 3, 5
    z, y = inputs(B, T)
    P = weights["random"]
    t = trainers("random")
    fh = t.forward(t_(z, torch_dev)).cpu().numpy()
    if case == "pitch_error_0":
        y[:, ::4, 18] = fh[:, ::4, 18]
    else:
        y[:, ::3, 19] = -0.75
    t.loss(t_(y, torch_dev))
    dz_dev = t.backward()
    by, total, d = tr.loss(y, fh)
    d_dev = t.dfeatures_hat.cpu().numpy()
    rows = np.s_[:, ::4, 18] if case == "pitch_error_0" else np.s_[:, ::3, 18]
    assert np.all(d_dev[rows] == 0.0) and np.all(d[rows] == 0.0)
    tr.check_tensor("dfhat", d_dev, d, 8 * U, case + ": ")                     # elementwise float32 from the same inputs: a few roundings of the largest element
    tr.check_tensor("loss", t.loss_by_batch.cpu().numpy(), by, tr.TOL["loss"], case + ": ")
    G, dz = tr.backward(P, tr.forward(P, z), d)
    tr.check_grads(host_grads(t), G, dz_dev.cpu().numpy(), dz, what=case + ": ")


# ---- independence and determinism -------------------------------------------------------------------------------------------------------------------------------
def test_a_sequence_does_not_depend_on_its_batch(torch_dev, trainers):
    """features_hat and dz_hat of a sequence, for the same rows of d features_hat, are bit-equal in batches of 1, 3 and 17 (sequences 0, 1, 2), and wherever the
    sequence stands in the batch: the 17 in reverse order puts sequence 0 alone in the second 16-sequence tile of the scans and sequence 16 first in the first"""
    T = 33
    z, _ = inputs(17, T)
    rng = np.random.default_rng(3)
    d = rng.standard_normal((17, 4 * T, 21)).astype(np.float32)
    t = trainers("model19")

    def run(order):
        fh = t.forward(t_(z[order], torch_dev))
        dz = t.backward(t_(d[order], torch_dev))
        return fh.cpu().numpy().view(np.uint32), dz.cpu().numpy().view(np.uint32)
    whole = run(np.arange(17))
    for B in (1, 3):
        for a, b in zip(run(np.arange(B)), whole):
            assert np.array_equal(a, b[:B]), f"a batch of {B} against the first {B} of 17"
    for a, b in zip(run(np.arange(17)[::-1]), whole):
        assert np.array_equal(a, b[::-1]), "the 17 sequences in reverse order"


def test_two_runs_and_a_smaller_handle_give_the_same_bits(torch_dev, trainers, weights):
    """a whole step twice from the same state; and (B, T) = (3, 5) on the (17, 33) handle against a handle opened at (3, 5)"""
    import torch
    z, y = inputs(3, 5)
    outs = []
    for key in (dict(), dict(), dict(B=3, T=5)):
        t = trainers("random", **key)
        p0 = t.flat_params.clone()
        t.flat_m.zero_(); t.flat_v.zero_(); t.n_steps = 0
        fh = t.forward(t_(z, torch_dev)); t.loss(t_(y, torch_dev)); dz = t.backward()
        grads = t.flat_grads.clone()
        t.flat_params.copy_(p0); t.n_steps = 0
        tot = t.train_step(t_(z, torch_dev), t_(y, torch_dev))
        outs.append([a.cpu().numpy().copy() for a in (fh, dz, grads, t.flat_grads, t.loss_by_batch, tot.reshape(1), t.flat_params, t.flat_m, t.flat_v, t.saved_x())])
        t.flat_params.copy_(p0); t.flat_m.zero_(); t.flat_v.zero_(); t.n_steps = 0
        torch.cuda.synchronize()
    for other in outs[1:]:
        for i, (a, b) in enumerate(zip(outs[0], other)):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"output {i} differs"
    assert np.array_equal(outs[0][2], outs[0][3]), "rade_train_dec_step's gradients are not those of the four calls"


# ---- the buffer contract ----------------------------------------------------------------------------------------------------------------------------------------
def test_guard_bands_inputs_and_refused_calls(torch_dev, weights):
    from radae_amd.abi import load_library
    L = load_library()
    B, T, n = 3, 5, L.rade_train_n_floats()
    assert n == tr.N_FLOATS
    z, y = inputs(B, T)
    h = L.rade_train_open(4, 8, 21, 0)
    assert h
    try:
        src = Dev(torch_dev)
        p_dev, z_dev, y_dev = src.put(tr.flatten(weights["random"])), src.put(z), src.put(y)
        band = lambda k, w=4: Band(1, k, k, w, torch_dev)
        fh, dfh, dz, g, x, loss = band(B * T * 84), band(B * T * 84), band(B * T * 80), band(n), band(B * T * 736), band(B + 1, 8)
        every = {"features_hat": fh, "dfeatures_hat": dfh, "dz_hat": dz, "grads": g, "x": x, "loss": loss}
        s = stream()
        # refused: nothing written, inputs untouched
        assert L.rade_train_dec_backward(h, p_dev.data_ptr(), None, g.ptr, dz.ptr, s) == -1, "backward ahead of any forward"
        assert L.rade_train_loss(h, y_dev.data_ptr(), dfh.ptr, loss.ptr, s) == -1, "loss ahead of any forward"
        for args in ((5, T), (B, 9), (B, 0), (0, T)):
            assert L.rade_train_dec_forward(h, p_dev.data_ptr(), z_dev.data_ptr(), args[0], args[1], fh.ptr, s) == -1, args
        assert L.rade_train_dec_forward(h, None, z_dev.data_ptr(), B, T, fh.ptr, s) == -1
        assert L.rade_train_dec_forward(h, p_dev.data_ptr(), None, B, T, fh.ptr, s) == -1
        assert L.rade_train_dec_forward(h, p_dev.data_ptr(), z_dev.data_ptr() + 2, B, T, fh.ptr, s) == -1, "a pointer off its element"
        assert L.rade_train_dec_forward(None, p_dev.data_ptr(), z_dev.data_ptr(), B, T, fh.ptr, s) == -1
        assert L.rade_train_open(0, 8, 21, 0) is None and L.rade_train_open(4, 8, 19, 0) is None
        sync()
        for k, b in every.items():
            b.untouched(k)
        # the calls
        assert L.rade_train_dec_forward(h, p_dev.data_ptr(), z_dev.data_ptr(), B, T, fh.ptr, s) == 0
        assert L.rade_train_dec_backward(h, p_dev.data_ptr(), None, g.ptr, dz.ptr, s) == -1, "backward with no gradient to start from"
        assert L.rade_train_loss(h, None, dfh.ptr, loss.ptr, s) == -1 and L.rade_train_loss(h, y_dev.data_ptr(), dfh.ptr, None, s) == -1
        assert L.rade_train_saved_x(h, x.ptr, s) == 0
        assert L.rade_train_loss(h, y_dev.data_ptr(), dfh.ptr, loss.ptr, s) == 0
        assert L.rade_train_dec_backward(h, p_dev.data_ptr(), None, None, dz.ptr, s) == -1
        assert L.rade_train_dec_backward(h, p_dev.data_ptr(), None, g.ptr, dz.ptr, s) == 0
        sync()
        for k, b in every.items():
            b.check(what=k)
        src.unchanged()
        S, by, total, d, G, dzr = tr.step_grads(weights["random"], z, y)
        tr.check_tensor("loss", loss.rows(np.float64)[0], np.append(by, total), tr.TOL["loss"])
        tr.check_grads(tr.unflatten(g.rows(np.float32)[0]), G, dz.rows(np.float32)[0].reshape(B, T, 80), dzr)
        # Adam: its four buffers, banded; a refused call first
        rng = np.random.default_rng(8)
        pb, gb, mb, vb = (band(n).fill(a.astype(np.float32)[None]) for a in (rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n), rng.random(n)))
        before = [b.rows() for b in (pb, gb, mb, vb)]
        assert L.rade_train_adam(h, pb.ptr, gb.ptr, mb.ptr, None, 3e-4, 0.2, 0.05, s) == -1 and L.rade_train_adam(h, pb.ptr, gb.ptr, mb.ptr, vb.ptr, 3e-4, 0.0, 0.05, s) == -1
        sync()
        assert all(np.array_equal(b.rows(), a) for b, a in zip((pb, gb, mb, vb), before))
        assert L.rade_train_adam(h, pb.ptr, gb.ptr, mb.ptr, vb.ptr, 3e-4, 0.2, 0.05, s) == 0
        sync()
        for k, b in (("params", pb), ("grads", gb), ("m", mb), ("v", vb)):
            b.check(what=k)
        assert np.array_equal(gb.rows(), before[1]) and not np.array_equal(pb.rows(), before[0])
    finally:
        L.rade_train_close(h)


def test_the_parameter_table_names_the_models_decoder(torch_dev):
    from radae_amd.train import param_table
    assert [(n, s) for n, _, s in param_table()] == tr.PARAM_TABLE
    off = 0
    for n, o, s in param_table():
        assert o == off
        off += int(np.prod(s))


# ---- Adam -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_adam_per_element(torch_dev, trainers):
    """one launch against the float64 formula from the same float32 inputs.  Roundings (rade_train.hip's header): m' carries at most 3 of magnitude |m| + |g|, and
    float(1 - 0.8) one more; the update 6 more; p' one.  Elements with v = 0 and g = 0 stay finite and do not move."""
    t = trainers("random")
    n = t.flat_params.numel()
    rng = np.random.default_rng(12)
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 2, n)).astype(np.float32)
    m = (0.5 * rng.standard_normal(n) * np.abs(g)).astype(np.float32)
    v = (rng.random(n) * g.astype(np.float64) ** 2).astype(np.float32)
    g[:100] = 0; m[:100] = 0; v[:100] = 0
    keep = [a.clone() for a in (t.flat_params, t.flat_grads, t.flat_m, t.flat_v)]
    for dst, a in zip((t.flat_params, t.flat_grads, t.flat_m, t.flat_v), (p, g, m, v)):
        dst.copy_(t_(a, torch_dev))
    t.n_steps = 6
    lr, bc1, bc2 = t.schedule()
    t.step()
    p1, m1, v1 = (a.cpu().numpy().astype(np.float64) for a in (t.flat_params, t.flat_m, t.flat_v))
    for dst, a in zip((t.flat_params, t.flat_grads, t.flat_m, t.flat_v), keep):
        dst.copy_(a)
    t.n_steps = 0
    P, Gd, M, V = (a.astype(np.float64) for a in (p, g, m, v))
    pr, mr, vr = tr.adam(P, Gd, M, V, lr, 7)
    assert abs(lr - 3e-4 / (1 + 2.5e-5 * 6)) < 1e-18 and abs(bc1 - (1 - 0.8 ** 7)) < 1e-15
    assert np.isfinite(p1).all() and np.array_equal(p1[:100], P[:100]) and np.all(m1[:100] == 0) and np.all(v1[:100] == 0)
    dm, dv = 4 * U * (np.abs(M) + np.abs(Gd)), 5 * U * (np.abs(V) + Gd * Gd)
    assert np.all(np.abs(m1 - mr) <= dm) and np.all(np.abs(v1 - vr) <= dv)
    denom = np.sqrt(vr) / np.sqrt(bc2) + tr.EPS
    upd = (lr / bc1) * mr / denom
    # d upd = (lr / bc1) (dm / denom + |m| d denom / denom^2), d denom = dv / (2 sqrt(v) sqrt(bc2)) where v > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        ddenom = np.where(vr > 0, dv / (2 * np.sqrt(vr) * np.sqrt(bc2)), 0.0)
    bound = (lr / bc1) * (dm / denom + np.abs(mr) * ddenom / denom ** 2) + 7 * U * np.abs(upd) + U * np.abs(pr)
    worst = np.max(np.abs(p1 - pr) / bound, where=bound > 0, initial=0.0)
    print(f"Adam: largest |d p| / bound {worst:.3f}")
    assert np.all(np.abs(p1 - pr) <= bound)


# ---- closing the loop -------------------------------------------------------------------------------------------------------------------------------------------
def test_ten_steps_on_one_batch(torch_dev, weights, tmp_path):
    """model19's decoder with every weight perturbed by a seeded 2 %, the target being the unperturbed decoder's output: the loss falls, and the first three losses,
    and parameter updates follow the float64 model's trajectory.  Per step: the loss within its bound; every gradient within TOL of the model's gradient AT THE
    DEVICE'S PARAMETERS of that step; and every element of every parameter's update against the free-running model's update within train_ref.UpdateBound, which
    carries a gradient error dg through Adam's m and v.  dg is TOL max|g| plus, from the second step on, the drift |model gradient at the device's parameters -
    model gradient at the model's parameters|, element by element: Adam's first update is lr g / (|g| + eps), a sign, so wherever float32 does not fix the sign of
    a small gradient the two parameter sets part by up to 2 lr, and the free-running gradients then differ by more than TOL (6e-5 of the largest element at the
    second step) with no error in any kernel.  The drift is the model's own figure, evaluated at the parameters the previous step's check has just held.  No element
    is left out: where a sign is not fixed the bound grows to the update's size by itself; at the first step, from the model alone, more than half of all
    elements are held to 1 % of the step.
    The learning rate: Adam's first updates move EVERY weight by about lr whatever its gradient, and the perturbation puts a weight 2 % of its size from the optimum --
    1.5e-3 at the median |w| = 0.076 of model19's decoder -- so steps of train.py's 3e-4 in 300 000 directions at once overshoot (the float64 model's loss goes from
    1.2e-2 to 1.16 in one step, and so does the device's).  LR = 2e-5 is 1 / 75 of the median perturbation; the float64 model's loss then falls from 1.24e-2 to 1.75e-3."""
    import torch
    from radae_amd import dnnw
    from radae_amd.engine import BatchEngine
    from radae_amd.train import DecoderTrainer
    B, T, LR = 8, 16, 2e-5
    rng = np.random.default_rng(77)
    z = rng.standard_normal((B, T, 80)).astype(np.float32)
    P0 = weights["model19"]
    y = tr.features_hat(tr.forward(P0, z)).astype(np.float32)
    P = {k: (v * (1 + 0.02 * rng.standard_normal(v.shape))).astype(np.float32).astype(np.float64) for k, v in P0.items()}
    t = DecoderTrainer(model_with(P), B=B, T=T, lr=LR)
    try:
        zd, yd = t_(z, torch_dev), t_(y, torch_dev)
        losses, updates, grads, at = [], [], [], []
        for k in range(10):
            before = t.flat_params.clone() if k < 3 else None
            losses.append(float(t.train_step(zd, yd)))
            if k < 3:
                at.append(tr.unflatten(before.cpu().numpy().astype(np.float64)))
                updates.append(tr.unflatten((t.flat_params - before).cpu().numpy().astype(np.float64)))
                grads.append(host_grads(t))
        fh = t.forward(zd)
        losses.append(float(t.loss(yd)))
        print("losses", " ".join(f"{v:.4e}" for v in losses))
        assert losses[10] < losses[0]
        # the float64 trajectory, three steps
        Pk = {k: v.copy() for k, v in P.items()}
        Mk, Vk = {k: np.zeros_like(v) for k, v in P.items()}, {k: np.zeros_like(v) for k, v in P.items()}
        UB = {k: tr.UpdateBound(v.shape) for k, v in P.items()}
        for k in range(3):
            Sk, _, total, dk, G, _ = tr.step_grads(Pk, z, y)
            # the target is another decoder's output, so the loss is a sum of squares of small differences of features_hat: to first order it moves by
            # sum |d total / d features_hat| x the error TOL allows features_hat, on top of TOL["loss"] for the sums
            bound = np.abs(dk).sum() * tr.TOL["features_hat"] * np.abs(Sk["out"]).max() + tr.TOL["loss"] * total
            print(f"step {k}: loss {losses[k]:.6e}, float64 model {total:.6e}, |d| / bound {abs(losses[k] - total) / bound:.3f}")
            assert abs(losses[k] - total) <= bound, (k, losses[k], total, bound)
            Gd = G if k == 0 else tr.step_grads(at[k], z, y)[4]            # the model's gradient at the device's parameters (step 0: the same parameters)
            fig = {n: tr.check_tensor(n, grads[k][n], Gd[n], tr.TOL["grad"], f"step {k}: ") for n in Pk}
            lr_t, s = tr.lr_at(LR, 2.5e-5, k), tr.lr_at(LR, 2.5e-5, k) / (1 - tr.BETAS[0] ** (k + 1))
            worst, where, tight, count = 0.0, None, 0, 0
            for name in Pk:
                want = Pk[name]
                (Pk[name], Mk[name], Vk[name]), bd = UB[name].step(want, G[name], Mk[name], Vk[name], lr_t, k + 1,
                                                                       np.abs(Gd[name] - G[name]) + tr.TOL["grad"] * np.abs(Gd[name]).max())
                ratio = np.abs(updates[k][name] - (Pk[name] - want)) / bd
                if ratio.max() > worst:
                    worst, where = float(ratio.max()), (name, np.unravel_index(int(np.argmax(ratio)), ratio.shape))
                tight += int(np.sum(bd <= 0.01 * s)); count += bd.size
            print(f"step {k}: gradients at most {max(f[0] for f in fig.values()):.2e} of TOL {tr.TOL['grad']:.1e}; updates at most {worst:.3f} of their bound "
                  f"({where[0]}{list(map(int, where[1]))}); {tight / count:.3f} of the elements held to 1 % of the step")
            assert worst <= 1.0, (k, where, worst)
            assert k or tight > count / 2
        # the trained decoder as a blob the batch engine loads: rade_batch_decode against the float64 model of the blob's own (quantised) weights
        path = str(tmp_path / "trained.bin")
        t.save_blob(path)
        eng = BatchEngine(B, max_tx_mf=(T + 2) // 3, blob=path)
        try:
            out = eng.decode(zd, 84).cpu().numpy()
        finally:
            eng.close()
        # ... and against the trainer's own forward to the int8 quantisation of write_blob, measured on the CPU with core_ref: the float64 model of the saved blob
        # against the float64 model of the float32 weights it was written from, 2 times that allowed (a decoder trained without quantisation noise is not on
        # the int8 grid, unlike the shipped one, whose blob re-quantises to itself: its figure would be 0, so the figure is taken for the blob at hand)
        dec, flt = core_ref.Decoder(dnnw.load_model(path)), core_ref.Decoder(t.to_model())
        fhh = fh.cpu().numpy().reshape(B, T, 84)
        for b in range(2):
            dec.reset(); flt.reset()
            want_q, want_f = dec.run(z[b])[0], flt.run(z[b])[0]
            assert core_ref.passes_rms_criterion(out[b], want_q), b
            quant = np.abs(want_q - want_f).max()
            print(f"sequence {b}: int8 quantisation moves the output by {quant:.3e}; the device's two decoders differ by {np.abs(out[b] - fhh[b]).max():.3e}")
            assert np.abs(out[b] - fhh[b]).max() <= 2 * quant
    finally:
        t.close()


# ---- the autograd wrapper ---------------------------------------------------------------------------------------------------------------------------------------
def test_decoder_apply_is_the_direct_call(torch_dev, trainers, model_steps):
    import torch
    from radae_amd.train import decoder_apply
    z, y, S, by, total, d, G, dz = model_steps("random", 3, 5)
    t = trainers("random")
    zt = t_(z, torch_dev).requires_grad_(True)
    w = t_(np.random.default_rng(2).standard_normal((3, 20, 21)).astype(np.float32), torch_dev)
    (decoder_apply(t, zt) * w).sum().backward()
    g_auto, grads_auto = zt.grad.cpu().numpy(), t.flat_grads.clone()
    t.forward(t_(z, torch_dev))
    g_direct = t.backward(w).cpu().numpy()
    assert np.array_equal(g_auto.view(np.uint32), g_direct.view(np.uint32)) and torch.equal(grads_auto, t.flat_grads)
    G64, dz64 = tr.backward(weights_of(t), S, w.cpu().numpy().astype(np.float64))
    tr.check_tensor("dz_hat", g_auto, dz64, tr.TOL["dz_hat"])


def weights_of(trainer):
    return {k: v.cpu().numpy().astype(np.float64) for k, v in trainer.params.items()}


# ---- the command line -------------------------------------------------------------------------------------------------------------------------------------------
def test_cli_train_decoder_writes_a_blob_the_engine_loads(torch_dev, tmp_path, capsys):
    """`cli train_decoder` over a small file pair: 6 sequences of 16 frames (T = 4), batches of 2 with the ragged rest dropped, two epochs; the blob it writes loads,
    its decoder has moved, its encoder has not, and the logged epoch losses are those of DecoderTrainer.train_step over the same batches"""
    from radae_amd import abi, cli, dnnw, train
    rng = np.random.default_rng(5)
    z = rng.standard_normal((27, 80)).astype(np.float32)
    f = np.zeros((27 * 4, 36), np.float32)
    f[:, :20] = rng.standard_normal((27 * 4, 20))
    z.tofile(tmp_path / "z.f32"); f.tofile(tmp_path / "f.f32")
    out = str(tmp_path / "out.bin")
    assert cli.main(["train_decoder", abi.DEFAULT_BLOB, str(tmp_path / "z.f32"), str(tmp_path / "f.f32"), out, "--sequence-length", "16", "--batch-size", "2",
                     "--epochs", "2", "--lr", "1e-5", "--auxdata", "--seed", "4"]) == 0
    logged = [ln for ln in capsys.readouterr().err.splitlines() if ln.startswith("epoch") and "batch" not in ln]
    assert len(logged) == 2
    m0, m1 = dnnw.load_model(abi.DEFAULT_BLOB), dnnw.load_model(out)
    assert np.array_equal(m0.enc_dense1.w, m1.enc_dense1.w) and not np.array_equal(m0.dec_output.w, m1.dec_output.w)
    zs, fs = train.load_sequences(str(tmp_path / "z.f32"), str(tmp_path / "f.f32"), 16, True, 4)
    assert zs.shape == (6, 4, 80) and fs.shape == (6, 16, 21)
    t = train.DecoderTrainer(abi.DEFAULT_BLOB, B=2, T=4, lr=1e-5)
    try:
        g = np.random.default_rng(4)
        for line in logged:
            tot = [float(t.train_step(t_(zs[i], torch_dev), t_(fs[i], torch_dev))) for i in train.epoch_batches(6, 2, g)]
            assert len(tot) == 3 and abs(float(line.split("total_loss=")[1]) - np.mean(tot)) <= 1e-5 * np.mean(tot), line
    finally:
        t.close()
