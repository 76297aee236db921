#!/usr/bin/env python3
"""Time of one training step of the decoder on the device (rade_train_dec_step: rade_train.hip) per phase -- forward GEMMs, forward scans, loss, backward scans, backward
GEMMs (with the activation derivatives and the folds of the weight gradients), Adam -- by the handle's own HIP events (rade_train_profile), at two shapes:
    default   B = 32,  T = 64    train.py's batch size and sequence length (256 frames)
    large     B = 512, T = 100   compare_models.sh:11
each in alternating rounds in one process next to torch-ROCm eager autograd of a plain torch restatement of the same decoder on the same device (torch.nn.GRU where it
runs there, else the cell written out step by step; which one is recorded), forward + loss + backward + torch.optim.Adam, timed by HIP events around the step.
Derived: the share of the 157 TFLOP/s f32 matrix peak the GEMM phases reach, and the cycles per recurrence step of both scans at 2.4 GHz (one workgroup per 16
sequences, all resident at once: a launch's time is T steps) beside the 590 cycles of the inference scan k_gru_scan.  DESIGN.md quotes the medians.

    python3 tools/time_train.py [--rounds 5] [--reps 3] [--out profiles/time_train.json]
"""
import ctypes as C
import os
import sys


REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
SHAPES = {"default": (32, 64), "large": (512, 100)}
PHASES = ("forward_gemm", "forward_scan", "loss", "backward_scan", "backward_gemm", "adam")
GRU_IN = (96, 224, 352, 480, 608)
F32_MATRIX_PEAK, CLOCK_HZ = 157e12, 2.4e9


def forward_gemm_flops(M):
    return 2.0 * M * (96 * 80 + sum(288 * k + 96 * 96 + 32 * 2 * (k + 96) for k in GRU_IN) + 84 * 736)


def torch_decoder(P, grus):
    """the same graph in plain torch (radae_base.py:333-354 with n() = the identity) over a dict of parameter tensors; grus: five torch.nn.GRU modules holding the
    GRU weights, or None for the cell written out over P's"""
    import torch

    def gru(x, l):
        if grus is not None:
            return grus[l](x)[0]
        w_ih, w_hh, b_ih, b_hh = (P[f"dec_gru[{l}].{k}"] for k in ("w_ih", "w_hh", "b_ih", "b_hh"))
        gi, h, hs = x @ w_ih.T + b_ih, torch.zeros(x.shape[0], 96, device=x.device), []
        for t in range(x.shape[1]):
            gh = h @ w_hh.T + b_hh
            r, u = torch.sigmoid(gi[:, t, :96] + gh[:, :96]), torch.sigmoid(gi[:, t, 96:192] + gh[:, 96:192])
            n = torch.tanh(gi[:, t, 192:] + r * gh[:, 192:])
            h = (1 - u) * n + u * h
            hs.append(h)
        return torch.stack(hs, 1)

    def fwd(z):
        x = torch.tanh(z @ P["dec_dense1.w"].T + P["dec_dense1.b"])
        for l in range(5):
            h = gru(x, l)
            x = torch.cat([x, h * torch.sigmoid(h @ P[f"dec_glu[{l}].w"].T)], -1)
            xp = torch.cat([torch.zeros_like(x[:, :1]), x[:, :-1]], 1)
            w = P[f"dec_conv[{l}].w"]
            x = torch.cat([x, torch.tanh(xp @ w[:, :, 0].T + x @ w[:, :, 1].T + P[f"dec_conv[{l}].b"])], -1)
        out = x @ P["dec_output.w"].T + P["dec_output.b"]
        return out.reshape(z.shape[0], 4 * z.shape[1], 21)
    return fwd


def torch_loss(y, p):
    import torch
    ceps, pitch, corr = p[..., :18] - y[..., :18], 2 * (p[..., 18:19] - y[..., 18:19]), p[..., 19:20] - y[..., 19:20]
    pw, data = torch.relu(y[..., 19:20] + 0.5) ** 2, p[..., 20:21] - y[..., 20:21]
    return torch.mean(ceps ** 2 + 3. * (10 / 18) * torch.abs(pitch) * pw + (1 / 18) * corr ** 2 + (0.5 / 18) * data ** 2, dim=-1).mean(dim=-1).mean()


def main():
    import stage_timing as stg
    import torch
    from radae_amd.train import DecoderTrainer
    a = stg.parser(rounds=5, reps=3).parse_args()
    dev = torch.device("cuda", 0)
    out = {"rounds": a.rounds, "reps": a.reps, "f32_matrix_peak_tflops": F32_MATRIX_PEAK / 1e12, "clock_ghz": CLOCK_HZ / 1e9, "inference_scan_cycles_per_step": 590,
           "shapes": {}}
    for name, (B, T) in SHAPES.items():
        t = DecoderTrainer(None, B=B, T=T, lr=1e-6)
        g = torch.Generator(device=dev); g.manual_seed(1)
        z = torch.randn((B, T, 80), generator=g, device=dev)
        y = torch.randn((B, 4 * T, 21), generator=g, device=dev)
        P = {k: v.clone().requires_grad_(True) for k, v in t.params.items()}
        grus, why = [torch.nn.GRU(k, 96, batch_first=True).to(dev) for k in GRU_IN], ""
        with torch.no_grad():
            for l, m in enumerate(grus):
                for dst, k in ((m.weight_ih_l0, "w_ih"), (m.weight_hh_l0, "w_hh"), (m.bias_ih_l0, "b_ih"), (m.bias_hh_l0, "b_hh")):
                    dst.copy_(P[f"dec_gru[{l}].{k}"])
        try:
            torch_loss(y, torch_decoder(P, grus)(z)).backward(); torch.cuda.synchronize()
        except Exception as e:                                       # torch.nn.GRU's kernels do not run here: the cell step by step
            grus, why = None, repr(e)[:200]
        use_nn_gru = grus is not None
        fwd = torch_decoder(P, grus)
        opt = torch.optim.Adam([v for k, v in P.items() if not (use_nn_gru and "gru" in k)] + [q for m in (grus or []) for q in m.parameters()],
                               lr=1e-6, betas=(0.8, 0.95), eps=1e-8)

        def torch_step():
            opt.zero_grad(set_to_none=True)
            torch_loss(y, fwd(z)).backward()
            opt.step()

        phase_ms = {k: [] for k in PHASES}

        def device_step(reps):
            """`reps` steps under the handle's events: ms per step of the whole, the phases kept aside"""
            ms = (C.c_double * 6)()
            assert t.L.rade_train_profile(t.h, 1) == 0
            for _ in range(reps):
                t.train_step(z, y)
            assert t.L.rade_train_profile_get(t.h, ms) > 0 and t.L.rade_train_profile(t.h, 0) == 0
            for k, v in zip(PHASES, ms):
                phase_ms[k].append(v / reps)
            return sum(ms) / reps

        calls = {"step": lambda: t.train_step(z, y), "phases": None, "torch_eager": torch_step}
        stg.warm({k: v for k, v in calls.items() if v})
        res = stg.rounds(calls, a.rounds, a.reps, clocks={"phases": lambda fn, reps: device_step(reps)})
        s = stg.stats(res)
        ph = stg.stats(phase_ms)
        fl = forward_gemm_flops(B * T)
        out["shapes"][name] = {
            "B": B, "T": T, "ms_per_step": s, "ms_per_phase": ph, "torch_gru": "torch.nn.GRU" if use_nn_gru else "cell by cell: " + why,
            "torch_over_device": s["torch_eager"]["median"] / s["step"]["median"],
            "forward_gemm_tflops": fl / (ph["forward_gemm"]["median"] * 1e-3) / 1e12, "backward_gemm_tflops": 2 * fl / (ph["backward_gemm"]["median"] * 1e-3) / 1e12,
            "forward_gemm_share_of_peak": fl / (ph["forward_gemm"]["median"] * 1e-3) / F32_MATRIX_PEAK,
            "backward_gemm_share_of_peak": 2 * fl / (ph["backward_gemm"]["median"] * 1e-3) / F32_MATRIX_PEAK,
            "forward_scan_cycles_per_step": ph["forward_scan"]["median"] * 1e-3 * CLOCK_HZ / (5 * T),
            "backward_scan_cycles_per_step": ph["backward_scan"]["median"] * 1e-3 * CLOCK_HZ / (5 * T),
            "bounding_phase": max(PHASES, key=lambda k: ph[k]["median"])}
        t.close()
    stg.emit(out, a.out)


if __name__ == "__main__":
    main()
