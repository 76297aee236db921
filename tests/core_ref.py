"""The core network in float64: a numpy restatement of the reference's CoreDecoderStatefull (radae_base.py:358-430) and core encoder (:223-286), built from a
dnnw.Model, one 40 ms step per call.  It is the model every device decoder and encoder is held to PER ELEMENT (tests/test_core_model_gpu.py), and is itself held to
the golden traces, the exporter's fixture and the C oracle (tests/test_core_ref_host.py).  numpy only; holds no fixtures.

Also here: the probe blobs that make the decoder's concat buffer x[736] visible in features_out (window, holes), or that fix every unique-word decision (aux);
the row / reset / chunk bookkeeping of a receiver trace; and the per-element comparison with the message a failure prints.

Layout of the decoder's concat buffer x (DenseNet style, every layer reads all columns before its own):
    [0, 96) dense1;  then for l = 0..4 at base 96 + 128 l:  [base, base + 96) GLU l + 1 (of GRU l + 1),  [base + 96, base + 128) conv l + 1.
"""
import copy

import numpy as np

from radae_amd import dnnw

DEC_W = 736                      # 96 + 5 (96 + 32)
ENC_W = 864                      # 64 + 5 (64 + 96)
N_WINDOWS = 9
UW_COL = 20                      # the unique-word column of a decoder row (rade_rx.hip: f84[r * 84 + 20] > 0)


def _sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1 / (1 + e), e / (1 + e))


def _f64(a):
    return np.asarray(a, np.float64)


class _Gru:
    def __init__(self, g):
        self.w_ih, self.w_hh, self.b_ih, self.b_hh = _f64(g.w_ih), _f64(g.w_hh), _f64(g.b_ih), _f64(g.b_hh)
        self.H = self.w_hh.shape[1]

    def step(self, h, x):
        """torch.nn.GRU cell, gate order r, z, n:  h' = (1 - z) n + z h"""
        H = self.H
        gi, gh = self.w_ih @ x + self.b_ih, self.w_hh @ h + self.b_hh
        r = _sigmoid(gi[:H] + gh[:H])
        z = _sigmoid(gi[H:2 * H] + gh[H:2 * H])
        n = np.tanh(gi[2 * H:] + r * gh[2 * H:])
        return (h - n) * z + n


class _Conv:
    """causal two-tap convolution: tanh(W[:, :, 0] x[t - dilation] + W[:, :, 1] x[t] + b)"""

    def __init__(self, c):
        self.w0, self.w1, self.b, self.dil = _f64(c.w[:, :, 0]), _f64(c.w[:, :, 1]), _f64(c.b), int(c.dilation)

    def new_history(self):
        return [np.zeros(self.w0.shape[1]) for _ in range(self.dil)]

    def step(self, hist, x):
        y = np.tanh(self.w0 @ hist[0] + self.w1 @ x + self.b)
        hist.pop(0); hist.append(x.copy())
        return y


class Decoder:
    """z_hat[80] -> (row[84], x[736]); x is returned so that a failure can name the layer"""

    def __init__(self, model):
        self.d1w, self.d1b = _f64(model.dec_dense1.w), _f64(model.dec_dense1.b)
        self.gru = [_Gru(g) for g in model.dec_gru]
        self.glu = [_f64(g.w) for g in model.dec_glu]
        self.conv = [_Conv(c) for c in model.dec_conv]
        self.ow, self.ob = _f64(model.dec_output.w), _f64(model.dec_output.b)
        self.reset()

    def reset(self):
        self.h = [np.zeros(96) for _ in range(5)]
        self.hist = [c.new_history() for c in self.conv]

    def step(self, z_hat):
        x = np.zeros(DEC_W)
        x[:96] = np.tanh(self.d1w @ _f64(z_hat).ravel() + self.d1b)
        n = 96
        for l in range(5):
            self.h[l] = h = self.gru[l].step(self.h[l], x[:n])
            x[n:n + 96] = h * _sigmoid(self.glu[l] @ h)
            n += 96
            x[n:n + 32] = self.conv[l].step(self.hist[l], x[:n])
            n += 32
        return self.ow @ x + self.ob, x

    def run(self, rows, resets=None):
        """rows [n, 80], resets [n] (a true flag resets the state BEFORE that row) -> (out [n, 84], x [n, 736])"""
        rows = np.asarray(rows).reshape(-1, 80)
        out, xs = np.zeros((len(rows), self.ow.shape[0])), np.zeros((len(rows), DEC_W))
        for i, z in enumerate(rows):
            if resets is not None and resets[i]:
                self.reset()
            out[i], xs[i] = self.step(z)
        return out, xs


class Encoder:
    """features[84] -> z[80] (bottleneck 3: linear; bottleneck 1: tanh)"""

    def __init__(self, model):
        self.d1w, self.d1b = _f64(model.enc_dense1.w), _f64(model.enc_dense1.b)
        self.gru = [_Gru(g) for g in model.enc_gru]
        self.conv = [_Conv(c) for c in model.enc_conv]
        assert tuple(c.dil for c in self.conv) == dnnw.ENC_DILATION
        self.zw, self.zb = _f64(model.enc_zdense.w), _f64(model.enc_zdense.b)
        self.reset()

    def reset(self):
        self.h = [np.zeros(64) for _ in range(5)]
        self.hist = [c.new_history() for c in self.conv]

    def step(self, features, bottleneck=3):
        x = np.zeros(ENC_W)
        x[:64] = np.tanh(self.d1w @ _f64(features).ravel() + self.d1b)
        n = 64
        for l in range(5):
            self.h[l] = x[n:n + 64] = self.gru[l].step(self.h[l], x[:n])
            n += 64
            x[n:n + 96] = self.conv[l].step(self.hist[l], x[:n])
            n += 96
        z = self.zw @ x + self.zb
        return np.tanh(z) if bottleneck == 1 else z

    def run(self, feats, bottleneck=3):
        return np.stack([self.step(f, bottleneck) for f in feats])


# ---- rows, calls and resets -------------------------------------------------------------------------------------------------------------------------------------
def rows_to_features(rows):
    """decoder rows [n_calls, 3, 84] (or [3 n_calls, 84]) -> what a valid call writes: [n_calls, 432] = 12 frames x 36, the first 20 of each 21 columns of a
    row, the 16 pad columns exactly 0"""
    r = np.asarray(rows)
    r = r.reshape(-1, 3, 4, 21)[..., :20]
    out = np.zeros((r.shape[0], 12, 36), r.dtype)
    out[:, :, :20] = r.reshape(-1, 12, 20)
    return out.reshape(-1, 432)


def resets_from_trace(ret, state_before, state_after):
    """one flag per VALID call of a receiver trace: the first valid call after a candidate -> sync transition resets the decoder before its first row
    (rade_rx.hip: dec_reset_pending set at sync entry, taken by the next valid call's row 0).  States: 0 search, 1 candidate, 2 sync."""
    flags, pending = [], False
    for r, sb, sa in zip(ret, state_before, state_after):
        if sb == 1 and sa == 2:
            pending = True
        if r & 1:
            flags.append(pending); pending = False
    return np.array(flags, bool)


def row_resets(call_resets):
    """per-call flags -> per-row flags (three rows per call, the flag on the first)"""
    out = np.zeros(3 * len(call_resets), bool)
    out[::3] = call_resets
    return out


def segments(row_flags):
    """[(lo, hi)] of the runs of rows between resets"""
    cuts = sorted(set([0] + [int(i) for i in np.flatnonzero(row_flags)] + [len(row_flags)]))
    return [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]


def uw_errors_from_rows(tr, out_rows):
    """the trace's uw_errors of every call whose state_before is sync, from decoder rows [3 n_valid, 84] (radae_rxe.py:220-224, :305-312): the sum restarts at
    sync entry and at every call with synced_count % 8 == 0, and a valid call adds its three rows' `row[20] > 0`.  Returns (call indices, expected)."""
    idx, want, uw, k = [], [], 0, 0
    for c in range(len(tr["ret"])):
        sb, sa, ret = int(tr["state_before"][c]), int(tr["state_after"][c]), int(tr["ret"][c])
        if sb == 1 and sa == 2:
            uw = 0
        if sb == 2 and int(tr["synced_count"][c]) % 8 == 0:
            uw = 0
        if ret & 1:
            uw += int(np.sum(out_rows[3 * k:3 * k + 3, UW_COL] > 0)); k += 1
        if sb == 2:
            idx.append(c); want.append(uw)
    return np.array(idx, int), np.array(want, int)


def chunk_plan(tr, dec_rows=48, round_calls=128, per_call=False):
    """Where the receiver kernel runs its decoder stage, from a trace (rade_rx.hip: prepare_next's `need`, rx2_decode_pending): a stream's valid calls queue three
    rows each; the queue is decoded ahead of a synchronised call whose synced_count becomes a multiple of 8 (the unique-word check), when three more rows would
    not fit dec_rows, at the end of a launch (round_calls calls; per_call: every call is its own launch), and it is cut into chunks of at most 12 rows.
    Returns (pos [3 n_valid, 2] = (row's position in its chunk, rows of that chunk), sizes of the queues decoded)."""
    pos, queues, n = [], [], 0

    def flush():
        nonlocal n
        if n:
            queues.append(n)
            for i in range(n):
                pos.append((i % 12, min(12, n - 12 * (i // 12))))
        n = 0
    for c in range(len(tr["ret"])):
        if per_call or (c and c % round_calls == 0):
            flush()
        if (int(tr["state_before"][c]) == 2 and int(tr["synced_count"][c]) % 8 == 0) or n + 3 > dec_rows:
            flush()
        if int(tr["ret"][c]) & 1:
            n += 3
    flush()
    return np.array(pos, int).reshape(-1, 2), queues


VISIBLE = np.array([j for j in range(84) if j % 21 != 20])      # the 80 columns of a decoder row that reach features_out (rows_to_features)


# ---- probe blobs ------------------------------------------------------------------------------------------------------------------------------------------------
def window_base(w):
    return min(84 * w, DEC_W - 84)


def select(model, x_cols, out_cols):
    """the model with an output layer that copies x[x_cols[i]] to output column out_cols[i]; every other weight is 0, the bias is 0 except column 20 -- the
    unique-word column the receiver reads -- which gets -4, so that no window ever fails whatever x holds there (|x| <= 1)"""
    m = copy.copy(model)
    W = np.zeros((84, DEC_W), np.float32)
    W[np.asarray(out_cols), np.asarray(x_cols)] = 1.0
    b = np.zeros(84, np.float32); b[UW_COL] = -4.0
    m.dec_output = dnnw.Dense(W, b)
    return m


def window(model, w):
    """select() of x[c0 .. c0 + 83] in order, c0 = window_base(w), w = 0..8"""
    return select(model, window_base(w) + np.arange(84), np.arange(84))


def hidden_columns():
    """The columns of x that no window shows in features_out: a valid call keeps the first 20 of each 21 columns of a row (rows_to_features), so a window hides
    x[c0 + 20], [c0 + 41], [c0 + 62], [c0 + 83] from the in-kernel decoder (the layer-wise and step decoders return whole rows).  35 columns, the last one, x[735],
    among them whatever the base of a contiguous window."""
    seen = set()
    for w in range(N_WINDOWS):
        seen |= set((window_base(w) + VISIBLE).tolist())
    return np.array(sorted(set(range(DEC_W)) - seen))


def holes(model):
    """select() of hidden_columns() into the first visible output columns: with the nine windows, every column of x reaches features_out"""
    h = hidden_columns()
    return select(model, h, VISIBLE[:len(h)])


def aux(model, bias):
    """the model with output row 20 made small (2^-6 of its weights: |w . x| <= sum |w| / 64 < 1 for the synthetic and the shipped blobs) and its bias +-4: every
    unique-word bit is right (-4) or wrong (+4) by a margin of at least 3"""
    m = copy.copy(model)
    W, b = model.dec_output.w.copy(), model.dec_output.b.copy()
    W[UW_COL] *= np.float32(2.0 ** -6); b[UW_COL] = np.float32(bias)
    assert np.abs(W[UW_COL]).sum() < 1.0
    m.dec_output = dnnw.Dense(W, b)
    return m


def write_probe(model, path):
    dnnw.write_blob(model, str(path))
    return str(path)


def column_name(c):
    """the layer a column of x belongs to"""
    if c < 96:
        return f"dense1[{c}]"
    l, r = divmod(c - 96, 128)
    return f"GLU {l + 1}[{r}]" if r < 96 else f"conv {l + 1}[{r - 96}]"


# ---- the per-element comparison ----------------------------------------------------------------------------------------------------------------------------------
def check_elements(door, blob, got, want, limit, out_cols=None, x_cols=None, stream=None, chunk_pos=None):
    """|got - want| <= limit for every row and column of [n, k] (limit a scalar or an array that broadcasts); returns max |got - want|.  out_cols[k]: the decoder-row
    column of each compared column (default 0..k-1); x_cols[k]: the column of x it shows, for a probe blob.  The failure names the door, the blob, the column (with
    its layer), the stream, the row and the row's position in its chunk."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (door, blob, got.shape, want.shape)
    err = np.abs(got - want)
    bad = ~(err <= limit)                                    # (a NaN is bad)
    if bad.any():
        lim = np.broadcast_to(np.asarray(limit, np.float64), err.shape)
        nan = bad & ~np.isfinite(err)
        r, c = np.argwhere(nan)[0] if nan.any() else np.unravel_index(int(np.argmax(np.where(bad, err / np.maximum(lim, 1e-300), -1.0))), err.shape)
        where = f"output column {c if out_cols is None else int(out_cols[c])}"
        if x_cols is not None and x_cols[c] is not None and x_cols[c] >= 0:
            where += f" = x[{int(x_cols[c])}], {column_name(int(x_cols[c]))}"
        pos = "" if chunk_pos is None else f", row {int(chunk_pos[r][0])} of a chunk of {int(chunk_pos[r][1])}"
        raise AssertionError(f"door {door}, blob {blob}: {where}, stream {stream}, row {r}{pos}: got {got[r, c]!r}, float64 model {want[r, c]!r}, "
                             f"|difference| {err[r, c]:.3e} > limit {lim[r, c]:.3e} ({int(bad.sum())} elements over)")
    return float(err.max()) if err.size else 0.0


def passes_rms_criterion(got, want):
    """the aggregate bar the suite has held every decoder to: rms < 1e-5 and max < 1e-4 over the 432-column features"""
    d = np.asarray(got, np.float64) - np.asarray(want, np.float64)
    return bool(np.sqrt(np.mean(d ** 2)) < 1e-5 and np.abs(d).max() < 1e-4)
