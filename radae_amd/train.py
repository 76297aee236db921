"""Training the decoder on the device: the Python side of rade_train_* (include/rade_batch.h; kernels in radae_amd/csrc/rade_train.hip).

DecoderTrainer holds the four flat float32 device buffers (parameters, gradients, Adam's m and v) and a handle that owns the activations: forward with saved
activations, the reference's distortion_loss (radae_base.py:50-68) with its gradient, back-propagation through time and Adam (train.py:147-150: betas (0.8, 0.95),
lr / (1 + decay step)).  decoder_apply makes the device decoder a differentiable torch function of z_hat, so an encoder and a channel written in torch can train through
it.  No CPU fallback: every call runs on the GPU through libradehip.so.

Deviations from the reference: the uniform noise of n() is left out (its clamp is the identity here); the GLU's effective weight is trained directly, and
weight_norm_grads gives the gradients of the reference's (g, v) parametrisation to a caller that keeps it.  Not here: the encoder, the channel's backward pass,
tqdm, the plots and .pth checkpoints.  load_sequences / epoch_batches / train_decoder restate the data handling of dataset.py:53-64, :105-110 and the loop of
train.py:240-287 for `cli train_decoder`; the shuffle and the aux bits come from a seeded numpy generator where the reference draws unseeded.
"""
from __future__ import annotations

import copy
import ctypes as C

import numpy as np
import torch

from . import dnnw
from .abi import TRAIN_SYMBOLS, load_library as _lib  # noqa: F401

BETAS = (0.8, 0.95)


def param_table():
    """[(name, offset in floats, shape)] of the flat buffers, from the library"""
    L = _lib()
    out = []
    for i in range(L.rade_train_n_params()):
        name, off, rows, cols = C.c_char_p(), C.c_long(), C.c_int(), C.c_int()
        assert L.rade_train_param(i, C.byref(name), C.byref(off), C.byref(rows), C.byref(cols)) == 0
        n = name.value.decode()
        shape = (rows.value,) if n.endswith((".b", ".b_ih", ".b_hh")) else (rows.value, cols.value // 2, 2) if ".w" in n and "conv" in n else (rows.value, cols.value)
        out.append((n, off.value, shape))
    return out


def _member(model, name):
    """the array of a dnnw.Model that a table name stands for: 'dec_gru[2].w_ih' -> model.dec_gru[2].w_ih"""
    obj = model
    for part in name.split("."):
        if "[" in part:
            attr, idx = part[:-1].split("[")
            obj = getattr(obj, attr)[int(idx)]
        else:
            obj = getattr(obj, part)
    return obj


def weight_norm_grads(dW, g, v):
    """Gradients of the reference's weight-normalised GLU gate (radae_base.py:138: W = g v / ||v||, the norm over each output row) from the gradient dW of the
    effective weight, in double: returns (dg [out, 1], dv [out, in])."""
    dW, v = np.asarray(dW, np.float64), np.asarray(v, np.float64)
    g = np.asarray(g, np.float64).reshape(-1, 1)
    norm = np.sqrt((v * v).sum(axis=1, keepdims=True))
    dot = (dW * v).sum(axis=1, keepdims=True)
    return dot / norm, g / norm * (dW - dot / (norm * norm) * v)


class DecoderTrainer:
    """model_or_blob: a dnnw.Model, the path of a DNNw blob, or None for the shipped one.  B, T: the capacity; a call may use less."""

    def __init__(self, model_or_blob=None, B=32, T=64, n_features=21, lr=3e-4, lr_decay=2.5e-5, device=0):
        from .abi import DEFAULT_BLOB
        self.h = None                                               # (close() runs from __del__ even when what follows raises)
        self.L = _lib()
        self.model = model_or_blob if isinstance(model_or_blob, dnnw.Model) else dnnw.load_model(model_or_blob or DEFAULT_BLOB)
        self.max_B, self.max_T, self.nf, self.lr, self.lr_decay, self.n_steps = B, T, n_features, lr, lr_decay, 0
        self.dev = torch.device("cuda", device)
        self.h = self.L.rade_train_open(B, T, n_features, device)
        if not self.h:
            raise RuntimeError("rade_train_open failed (no GPU? libradehip.so has no CPU fallback)")
        self.table = param_table()
        n = self.L.rade_train_n_floats()
        host = np.zeros(n, np.float32)
        for name, off, shape in self.table:
            a = np.asarray(_member(self.model, name), np.float32)
            assert a.shape == shape, (name, a.shape, shape)
            host[off:off + a.size] = a.ravel()
        self.flat_params = torch.from_numpy(host).to(self.dev)
        self.flat_grads, self.flat_m, self.flat_v = (torch.zeros(n, dtype=torch.float32, device=self.dev) for _ in range(3))
        self.params = {name: self.flat_params[off:off + int(np.prod(shape))].view(shape) for name, off, shape in self.table}
        self.grads = {name: self.flat_grads[off:off + int(np.prod(shape))].view(shape) for name, off, shape in self.table}
        self.B = self.T = 0
        self.loss_by_batch = self.total = self.dfeatures_hat = None

    def close(self):
        if self.h:
            self.L.rade_train_close(self.h); self.h = None

    def __del__(self):
        self.close()

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    @staticmethod
    def _check(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc})")

    def forward(self, z_hat: torch.Tensor) -> torch.Tensor:
        """z_hat [B, T, 80] float32 (cuda) -> features_hat [B, 4 T, 21]; the activations stay in the handle for loss() and backward()"""
        assert z_hat.is_cuda and z_hat.dtype == torch.float32 and z_hat.dim() == 3 and z_hat.shape[2] == 80
        z_hat = z_hat.contiguous()
        B, T = z_hat.shape[:2]
        out = torch.empty((B, 4 * T, 21), dtype=torch.float32, device=self.dev)
        self._check(self.L.rade_train_dec_forward(self.h, self.flat_params.data_ptr(), z_hat.data_ptr(), B, T, out.data_ptr(), self._stream()), "rade_train_dec_forward")
        self.B, self.T = B, T
        return out

    def saved_x(self) -> torch.Tensor:
        x = torch.empty((self.B, self.T, 736), dtype=torch.float32, device=self.dev)
        self._check(self.L.rade_train_saved_x(self.h, x.data_ptr(), self._stream()), "rade_train_saved_x")
        return x

    def loss(self, features: torch.Tensor) -> torch.Tensor:
        """features [B, 4 T, n_features]: the total loss (a 0-d float64 tensor on the device); .loss_by_batch [B] and .dfeatures_hat [B, 4 T, 21] are kept"""
        assert features.is_cuda and features.dtype == torch.float32 and tuple(features.shape) == (self.B, 4 * self.T, self.nf), tuple(features.shape)
        features = features.contiguous()
        loss = torch.empty(self.B + 1, dtype=torch.float64, device=self.dev)
        d = torch.empty((self.B, 4 * self.T, 21), dtype=torch.float32, device=self.dev)
        self._check(self.L.rade_train_loss(self.h, features.data_ptr(), d.data_ptr(), loss.data_ptr(), self._stream()), "rade_train_loss")
        self.loss_by_batch, self.total, self.dfeatures_hat = loss[:self.B], loss[self.B], d
        return self.total

    def backward(self, dfeatures_hat: torch.Tensor | None = None) -> torch.Tensor:
        """fills .grads and returns dz_hat [B, T, 80]; dfeatures_hat None: the gradient loss() left"""
        p = None
        if dfeatures_hat is not None:
            assert dfeatures_hat.is_cuda and dfeatures_hat.dtype == torch.float32 and dfeatures_hat.numel() == self.B * self.T * 84
            dfeatures_hat = dfeatures_hat.contiguous(); p = dfeatures_hat.data_ptr()
        dz = torch.empty((self.B, self.T, 80), dtype=torch.float32, device=self.dev)
        self._check(self.L.rade_train_dec_backward(self.h, self.flat_params.data_ptr(), p, self.flat_grads.data_ptr(), dz.data_ptr(), self._stream()), "rade_train_dec_backward")
        return dz

    def schedule(self):
        """(lr, bias_correction1, bias_correction2) of the NEXT step, in double: train.py:148-150's LambdaLR steps once per batch"""
        k = self.n_steps + 1
        return self.lr / (1.0 + self.lr_decay * self.n_steps), 1.0 - BETAS[0] ** k, 1.0 - BETAS[1] ** k

    def step(self):
        """one Adam update from .grads"""
        lr, bc1, bc2 = self.schedule()
        self._check(self.L.rade_train_adam(self.h, self.flat_params.data_ptr(), self.flat_grads.data_ptr(), self.flat_m.data_ptr(), self.flat_v.data_ptr(), lr, bc1, bc2,
                                           self._stream()), "rade_train_adam")
        self.n_steps += 1

    def train_step(self, z_hat: torch.Tensor, features: torch.Tensor) -> torch.Tensor:
        """forward, loss, backward and Adam in one C call; returns the loss ahead of the update (0-d float64 on the device)"""
        assert z_hat.is_cuda and z_hat.dtype == torch.float32 and z_hat.dim() == 3 and z_hat.shape[2] == 80
        B, T = z_hat.shape[:2]
        assert features.is_cuda and features.dtype == torch.float32 and tuple(features.shape) == (B, 4 * T, self.nf)
        z_hat, features = z_hat.contiguous(), features.contiguous()
        loss = torch.empty(B + 1, dtype=torch.float64, device=self.dev)
        lr, bc1, bc2 = self.schedule()
        self._check(self.L.rade_train_dec_step(self.h, self.flat_params.data_ptr(), self.flat_grads.data_ptr(), self.flat_m.data_ptr(), self.flat_v.data_ptr(), z_hat.data_ptr(),
                                               features.data_ptr(), B, T, loss.data_ptr(), lr, bc1, bc2, self._stream()), "rade_train_dec_step")
        self.B, self.T, self.n_steps = B, T, self.n_steps + 1
        self.loss_by_batch, self.total = loss[:B], loss[B]
        return self.total

    def to_model(self) -> dnnw.Model:
        """the dnnw.Model given at construction with the decoder replaced by the trained one"""
        host = self.flat_params.cpu().numpy()
        m = copy.copy(self.model)
        m.dec_gru, m.dec_glu, m.dec_conv = [copy.copy(g) for g in m.dec_gru], [copy.copy(g) for g in m.dec_glu], [copy.copy(c) for c in m.dec_conv]
        m.dec_dense1, m.dec_output = copy.copy(m.dec_dense1), copy.copy(m.dec_output)
        for name, off, shape in self.table:
            a = host[off:off + int(np.prod(shape))].reshape(shape).copy()
            head, attr = name.rsplit(".", 1)
            setattr(_member(m, head), attr, a)
        return m

    def save_blob(self, path):
        dnnw.write_blob(self.to_model(), str(path))


class _DecoderApply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, trainer, z_hat):
        ctx.trainer = trainer
        return trainer.forward(z_hat)

    @staticmethod
    def backward(ctx, grad_out):
        return None, ctx.trainer.backward(grad_out)


def decoder_apply(trainer: DecoderTrainer, z_hat: torch.Tensor) -> torch.Tensor:
    """features_hat = decoder(z_hat) as a differentiable function of z_hat: its backward runs rade_train_dec_backward, which also fills trainer.grads.  One forward at a
    time per trainer: the activations live in its handle."""
    return _DecoderApply.apply(trainer, z_hat)


# ---- the host side of `cli train_decoder` ------------------------------------------------------------------------------------------------------------------------
def load_sequences(z_file, feature_file, sequence_length=256, auxdata=False, seed=0, num_features=36, num_used_features=20):
    """The reference's dataset (dataset.py:53-64, :105-110) for a decoder: the feature file as [frames, 36], its first 20 columns, with --auxdata one symbol of +-1
    held over every 4 frames as column 20; sequence i is frames [i L, (i + 1) L) and latent rows [i L / 4, (i + 1) L / 4) of z_file ([rows, 80], what --write_latent
    writes: one row per 4 frames).  A ragged tail is dropped.  Returns (z [N, L / 4, 80], features [N, L, 20 | 21]) float32."""
    if sequence_length <= 0 or sequence_length % 4:
        raise ValueError("sequence_length must be a positive multiple of 4 (one latent row decodes to 4 feature frames)")
    f = np.reshape(np.fromfile(feature_file, dtype=np.float32), (-1, num_features))[:, :num_used_features]
    if auxdata:
        rng = np.random.default_rng(seed)
        aux = np.zeros((f.shape[0], 1))
        first = 1.0 - 2.0 * (rng.random(f.shape[0] // 4) > 0.5)
        for i in range(4):
            aux[i:4 * len(first):4, 0] = first
        f = np.concatenate([f, aux], axis=1, dtype=np.float32)
    z = np.reshape(np.fromfile(z_file, dtype=np.float32), (-1, 80))
    T = sequence_length // 4
    n = min(f.shape[0] // sequence_length, z.shape[0] // T)
    return (np.ascontiguousarray(z[:n * T].reshape(n, T, 80)), np.ascontiguousarray(f[:n * sequence_length].reshape(n, sequence_length, f.shape[1]), dtype=np.float32))


def epoch_batches(n_sequences, batch_size, rng):
    """DataLoader(shuffle=True, drop_last=True) (train.py:120): index arrays of one epoch"""
    order = rng.permutation(n_sequences)
    return [order[i:i + batch_size] for i in range(0, n_sequences - batch_size + 1, batch_size)]


def train_decoder(model, z, features, out_blob, batch_size=32, epochs=1, lr=3e-4, lr_decay=2.5e-5, seed=0, log=print, log_interval=10):
    """train.py:240-287 for the decoder alone: every epoch a fresh shuffle, one rade_train_dec_step per batch, the running losses every log_interval batches as
    tepoch.set_postfix shows them (the sampled BER is not restated); writes the blob and returns the mean loss of every epoch."""
    N, T = z.shape[:2]
    if N < batch_size:
        raise ValueError(f"{N} sequences, fewer than one batch of {batch_size}")
    t = DecoderTrainer(model, B=batch_size, T=T, n_features=features.shape[2], lr=lr, lr_decay=lr_decay)
    rng = np.random.default_rng(seed)
    zd, fd = torch.from_numpy(z).to(t.dev), torch.from_numpy(features).to(t.dev)
    means = []
    try:
        for epoch in range(1, epochs + 1):
            running = previous = 0.0
            batches = epoch_batches(N, batch_size, rng)
            for i, idx in enumerate(batches):
                idx = torch.from_numpy(idx).to(t.dev)
                running += float(t.train_step(zd[idx], fd[idx]))
                if (i + 1) % log_interval == 0:
                    log(f"epoch {epoch} batch {i + 1}/{len(batches)} current_loss={(running - previous) / log_interval:.6g} total_loss={running / (i + 1):.6g}")
                    previous = running
            means.append(running / len(batches))
            log(f"epoch {epoch} total_loss={means[-1]:.6g}")
        t.save_blob(out_blob)
    finally:
        t.close()
    return means
