// rade_bpf_fir.h -- the 101-tap FIR of complex_bpf (dsp.py:39-102) on the matrix cores: bpf_stage_planes, bpf_load_taps, bpf_fir_tile.  The project's ONE FIR
// arithmetic, included by every translation unit that filters: rade_rx.hip (through rade_bpf.h: the pre-pass kernel k_bpf_fir and the receiver's own off-grid
// filtering) and rade_file.hip (the whole-file filter of the stored-file receiver, k_file_bpf).  Needs rade_devutil.h (f16x8, f32x4, wave_max_f32).
#ifndef RADE_BPF_FIR_H
#define RADE_BPF_FIR_H
// y[i] = sum_t h[t] w[i + t] over a window w of baseband samples is the product of the Toeplitz matrix T[r][m] = h[m - r] (16 x 128, taps padded
// with zeros) with the Hankel matrix U[m][q] = w[16 q + m]: Y[r][q] = y[16 q + r], one 16 x 16 tile = 256 consecutive outputs.  On
// v_mfma_f32_16x16x32_f16: T is the A operand (two binary16 planes of 2^10 h, a constant table: rd_bpf16_table_fill), U the B operand -- its
// fragment for (column q, k-group g, k-step ks) is EIGHT CONSECUTIVE window samples starting at 16 q + 32 ks + 8 g, one aligned 16-byte LDS read
// from a plane -- real and imaginary parts as separate planes, each split hi + lo (22 bits, one power-of-two scale per block from its largest
// component): hi hi + hi lo + lo hi in f32, 24 matrix instructions per tile against 51,712 vector FMAs.  The vector FIR was bound by LDS reads
// (every thread re-read its sliding window); this form reads each plane entry 8 times instead of 101.
#define BPF_NPL 1408                   /* halfs per plane: five tiles of 256 outputs + the 127 samples the last rows reach beyond */
#define BPF_TILES(n) (((n) + 255) >> 8)
struct BpfLds {                        // 11,264 B: exactly the receiver's xm work area
    __attribute__((aligned(16))) _Float16 rh[BPF_NPL], rl[BPF_NPL], ih[BPF_NPL], il[BPF_NPL];
};
// The window [memory (102) | block (n)] into the four planes, entry i of it at plane index i - o (o = 2 before a stream's first call, whose memory is two
// samples shorter: dsp.py:55; entries below o are dropped): thread tid brings head = entry tid (tid < 102) and body[q] = entry 102 + tid + 256 q, ZERO
// beyond the block -- all loaded by the caller in one batch, so that a workgroup pays one memory round trip for its window and not one per entry.
// Returns the factor that undoes the operand scales.  Every thread of the 256-thread workgroup calls this (two barriers inside); maxw is an LDS word.
// What a caller may rely on, X = the window's largest |component| with biased exponent e: both scales are powers of two, so 2^k x gives 2^k y bit for bit while
// e stays inside the clamp [32, 222], 2^-95 <= X < 2^96, where X lands in [2^7, 2^8) and a plane entry is good to 22 bits above a floor of 2^-32 X.  Below 2^-95 the
// scale stays 2^102: the floor stays 2^-32 x 2^-95 = 2^-127 absolute, a relative error that grows as the block fades.  Above 2^96 the scale stays 2^-88: the 22 bits
// hold while every entry is finite in binary16, X < 65520 x 2^88 (just under 2^104); beyond that the block's outputs are infinities and NaNs.  tests/bpf_ref.py counts it.
#define BPF_NQ 5                       /* body entries per thread: 5 x 256 >= the longest block (1152, the end-of-over frame on the transmit side) */
__device__ __forceinline__ float bpf_stage_planes(BpfLds *pl, unsigned *maxw, int tid, float2 head, const float2 (&body)[BPF_NQ], int o)
{
    float m = tid < 102 ? fmaxf(fabsf(head.x), fabsf(head.y)) : 0.0f;
#pragma unroll
    for (int q = 0; q < BPF_NQ; q++) m = fmaxf(m, fmaxf(fabsf(body[q].x), fabsf(body[q].y)));
    if (tid == 0) *maxw = 0u;
    __syncthreads();
    m = wave_max_f32(m);
    if ((tid & 63) == 0) atomicMax(maxw, __float_as_uint(m));
    __syncthreads();
    float sc, unsc;                                                                    // operand_scale (rade_devutil.h) is the clamp spoken of above; unsc: 2^(E - 7) from the samples, 2^-10 from the taps
    operand_scale<10>(*maxw, sc, unsc);
    auto put = [&](int w, float2 v) {
        const float xr = v.x * sc, xi = v.y * sc;
        const _Float16 h0 = (_Float16)xr, h1 = (_Float16)xi;
        pl->rh[w] = h0; pl->rl[w] = (_Float16)(xr - (float)h0); pl->ih[w] = h1; pl->il[w] = (_Float16)(xi - (float)h1);
    };
    if (tid < 102 && tid >= o) put(tid - o, head);
#pragma unroll
    for (int q = 0; q < BPF_NQ; q++) put(102 - o + tid + 256 * q, body[q]);
    if (tid < BPF_NPL - (102 + 256 * BPF_NQ)) put(102 + 256 * BPF_NQ + tid, make_float2(0.0f, 0.0f));      // the tail the last tile's rows reach into
    if (tid < o) put(BPF_NPL - o + tid, make_float2(0.0f, 0.0f));
    __syncthreads();
    return unsc;
}
// outputs 256 tile + 16 (lane & 15) + 4 (lane >> 4) + r, r = 0..3, of the staged window: (re[r], im[r]), still in operand scale
struct BpfTaps { f16x8 h[4], l[4]; };          // the lane's A fragments (rd_bpf16_table_fill): loaded once, ahead of the staging
__device__ __forceinline__ void bpf_load_taps(BpfTaps &t, const unsigned short *tab16, int lane)
{
    typedef const __attribute__((address_space(1))) f16x8 glb_f16x8_t;
#pragma unroll
    for (int ks = 0; ks < 4; ks++) { t.h[ks] = *(glb_f16x8_t *)(tab16 + (((size_t)ks * 2) * 64 + lane) * 8); t.l[ks] = *(glb_f16x8_t *)(tab16 + (((size_t)ks * 2 + 1) * 64 + lane) * 8); }
}
__device__ __forceinline__ void bpf_fir_tile(const BpfLds *pl, const BpfTaps &t, int tile, int lane, f32x4 &re, f32x4 &im)
{
    const f16x8 (&Ah)[4] = t.h, (&Al)[4] = t.l;
    const int w0 = 256 * tile + 16 * (lane & 15) + 8 * (lane >> 4);
    f32x4 a[6];
#pragma unroll
    for (int k = 0; k < 6; k++) a[k] = (f32x4){ 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
    for (int ks = 0; ks < 4; ks++) {
        const f16x8 brh = *(const f16x8 *)&pl->rh[w0 + 32 * ks], brl = *(const f16x8 *)&pl->rl[w0 + 32 * ks];
        const f16x8 bih = *(const f16x8 *)&pl->ih[w0 + 32 * ks], bil = *(const f16x8 *)&pl->il[w0 + 32 * ks];
        a[0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Al[ks], brh, a[0], 0, 0, 0);
        a[1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ah[ks], brl, a[1], 0, 0, 0);
        a[2] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ah[ks], brh, a[2], 0, 0, 0);
        a[3] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Al[ks], bih, a[3], 0, 0, 0);
        a[4] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ah[ks], bil, a[4], 0, 0, 0);
        a[5] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ah[ks], bih, a[5], 0, 0, 0);
    }
    re = (a[0] + a[1]) + a[2]; im = (a[3] + a[4]) + a[5];
}
#endif
