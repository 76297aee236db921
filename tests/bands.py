"""Banded buffers for the buffer-contract tests (include/rade_batch.h, "Buffers, strides and alignment").

A Band is ONE flat allocation of 32-bit words: a front guard, B rows `stride` elements apart (so there is a gap behind every row of `row` elements) and a
back guard.  Every word starts as SENTINEL, a float32 NaN with a payload that neither a kernel nor a reference produces.  After a call, check() tells
    (a) a write outside the rows (guards, gaps) -- the first stream, the offset and how many words were hit,
    (b) a word of a row's written extent that was never written,
    (c) a write into the part of a row the header documents as not written (rows past n_valid, frame-loss entries past n_hat - start, unscored streams).
The guards are at least one stride and at least 4096 bytes each, so a whole stray tile lands inside the allocation.  Works on numpy arrays (host buffers, the
CPU self-test in tests/test_host_cpu.py) and on torch tensors (device buffers); holds no fixtures."""
import numpy as np

SENTINEL = np.uint32(0xFFC0DEAD).view(np.int32).item()          # as float32: a NaN


class Band:
    def __init__(self, B, row, stride, elem_bytes, device=None, base_offset_bytes=0):
        """B rows of `row` elements of elem_bytes (a multiple of 4) at `stride` elements.  device: a torch device (None: numpy).
        base_offset_bytes: row 0 starts at this offset modulo 16 from a 16-byte boundary (a multiple of 4)."""
        assert B >= 1 and 0 <= row <= stride and elem_bytes % 4 == 0 and base_offset_bytes % 4 == 0
        self.B, self.row, self.stride, self.w = B, row, stride, elem_bytes // 4
        guard = max(stride * self.w, 1024)                        # words: >= one stride and >= 4096 bytes
        guard = (guard + 3) // 4 * 4
        self.front = guard + (base_offset_bytes % 16) // 4
        self.n_words = self.front + B * stride * self.w + guard
        if device is None:
            raw = np.empty(self.n_words + 4, np.int32)            # numpy promises no 16-byte alignment: find it
            skip = (-raw.ctypes.data % 16) // 4
            self.words = raw[skip:skip + self.n_words]
            self.words[:] = SENTINEL
            self._addr = self.words.ctypes.data
        else:
            import torch
            self.words = torch.full((self.n_words,), SENTINEL, dtype=torch.int32, device=device)
            self._addr = self.words.data_ptr()
        assert self._addr % 16 == 0

    @property
    def ptr(self):
        """address of row 0"""
        return self._addr + 4 * self.front

    def host(self):
        w = self.words
        return w if isinstance(w, np.ndarray) else w.cpu().numpy()

    def fill(self, values):
        """rows <- values [B, row] (any dtype of the element size); gaps and guards keep the sentinel"""
        v = np.ascontiguousarray(values).reshape(self.B, -1).view(np.int32)
        assert v.shape == (self.B, self.row * self.w), (v.shape, self.B, self.row * self.w)
        h = np.array(self.host())
        for b in range(self.B):
            s = self.front + b * self.stride * self.w
            h[s:s + self.row * self.w] = v[b]
        if isinstance(self.words, np.ndarray):
            self.words[:] = h
        else:
            import torch
            self.words.copy_(torch.from_numpy(h))
        return self

    def rows(self, dtype=np.int32):
        """[B, row] copy of the rows on the host"""
        h = self.host()
        out = np.stack([h[self.front + b * self.stride * self.w:self.front + (b * self.stride + self.row) * self.w] for b in range(self.B)])
        return out.view(dtype)

    def check(self, written=None, what="buffer"):
        """written: elements from the start of each row that the call must have written (None: the whole row; an int: every stream; B values).
        The rest of the row is documented as not written and must still hold the sentinel, like the gaps and guards."""
        h = self.host()
        wr = np.broadcast_to(np.asarray(self.row if written is None else written, np.int64), (self.B,))
        assert wr.min() >= 0 and wr.max() <= self.row, "written extent outside the row"
        outside = np.ones(self.n_words, bool)
        for b in range(self.B):
            s = self.front + b * self.stride * self.w
            outside[s:s + self.row * self.w] = False
        hit = np.flatnonzero(outside & (h != SENTINEL))
        if hit.size:                                               # (a)
            i = int(hit[0])
            if i < self.front:
                where = f"{self.front - i} words before row 0"
            else:
                b = min((i - self.front) // (self.stride * self.w), self.B - 1)
                where = f"stream {b}, word {i - self.front - b * self.stride * self.w} of its stride (row = {self.row * self.w} words)"
            raise AssertionError(f"{what}: {hit.size} words written outside the rows, the first at {where}")
        for b in range(self.B):
            s = self.front + b * self.stride * self.w
            r = h[s:s + self.row * self.w]
            n = int(wr[b]) * self.w
            miss = np.flatnonzero(r[:n] == SENTINEL)
            if miss.size:                                          # (b)
                raise AssertionError(f"{what}: stream {b}: {miss.size} words of the written extent ({n} words) were never written, the first at word {int(miss[0])}")
            extra = np.flatnonzero(r[n:] != SENTINEL)
            if extra.size:                                         # (c)
                raise AssertionError(f"{what}: stream {b}: {extra.size} words written in the part documented as not written, the first at word {n + int(extra[0])}")

    def untouched(self, what="buffer"):
        """nothing at all was written (a refused call)"""
        self.check(written=0, what=what)
