// rade_bpf.h -- the band-pass filter (complex_bpf, dsp.py:39-102): the arithmetic shared by the pre-pass kernel k_bpf_fir and the receiver's own off-grid
// filtering (bpf_stage_planes, bpf_load_taps, bpf_fir_tile), and the receiver's side of it (rx2_bpf_mem, rx2_bpf_own).  Part of rade_rx.hip's translation
// unit, behind RxShared2.  Members of RxShared2 it owns: xm (the planes overlay it, the call's filtered samples are left there), redi[14] (the block maximum).
//
// The filter is a stateful streaming FIR of the input: mix down with a running phase, 101 real taps, mix up.  Nothing in it depends on the sync
// state machine, so it runs as a bulk pre-pass over all the samples of a rade_batch_rx invocation (k_bpf_chain + k_bpf_fir) and the receiver
// kernel reads filtered samples.  What the reference's arithmetic does depend on is how the stream is cut into calls: the phase is a complex64
// carried from call to call (phase_vec = phase * phase_vec_exp[0:n], self.phase = phase_vec[-1]: dsp.py:70-71, :99).  The pre-pass therefore
// follows the reference's own partition: block 0 = the nin the stream's next call will consume (from its state record), every later block Nmf
// samples -- exact unless a timing slip changes nin INSIDE an invocation; from that call on the stream filters its own samples (rx2_bpf_own)
// until the invocation ends, and the next invocation's pre-pass starts from the state it left.  Either way every output sample is what
// complex_bpf.bpf would have produced for the stream's actual sequence of calls, from ONE arithmetic (bpf_stage_planes + bpf_fir_tile, shared by
// the pre-pass kernel and rx2_bpf_own; mixers without fused multiply-adds: cmul_nc), so cutting a stream into invocations differently cannot move a bit.
// The same kernels filter the transmit side (radae_txe.py:74-83, :130-132: the optional Tx band-pass filter, there followed by the magnitude clip).
//   chain[b] (float2 [chain_stride]): entry 0 = (nin0, mem_len0) as integer bits, entry 1 + k = the phase block k starts from.
// Memory quirk kept (dsp.py:55 against :96): the memory holds Ntap - 1 = 100 samples before the first call and Ntap + 1 = 102 after it while the
// strided window always starts at index 0, so outputs are delayed by two more samples from the second call on.


// ---- the 101-tap FIR on the matrix cores (shared by the pre-pass kernel, the receiver's own off-grid filtering and the whole-file filter of rade_file.hip: one arithmetic) ----
#include "rade_bpf_fir.h"

// baseband sample q of the invocation (x[q] times the phase of its block), q >= -102: the filter memory a stream needs when it leaves the grid or
// the launch ends; negative q reaches into the memory the invocation started with
__device__ __forceinline__ float2 rx2_bpf_mem(const rd_sync_args &a, int b, int nin0, int q)
{
    const rd_rx_stream *st = a.st + b;
    if (q < 0) return make_float2(st->bpf.mem[102 + q][0], st->bpf.mem[102 + q][1]);
    const float2 *x = (const float2 *)a.rx + (size_t)b * a.rx_stride;
    const float2 *chain = (const float2 *)a.bpf_chain + (size_t)b * a.chain_stride;
    const int k = q < nin0 ? 0 : 1 + (q - nin0) / RD_NMF, sk = k ? nin0 + (k - 1) * RD_NMF : 0;
    return cmul_nc(x[q], cmul_nc(chain[1 + k], ld2(a.tab->bpf_E, q - sk)));
}

// One call's filtering by the stream's own workgroup (off the grid): the pre-pass's arithmetic on the stream's actual call.  Cold path; the filter
// memory lives in the stream record between calls.
__device__ __forceinline__ void rx2_bpf_own(RxShared2 *sh, const rd_sync_args &a, int b, float2 *rxf, int cons0, int nin, int calls0)
{
    static_assert(sizeof(BpfLds) <= sizeof(sh->xm), "the planes overlay the xm work area");
    RxScalars *S = &sh->S;
    rd_rx_stream *st = a.st + b;
    const rd_tables *tab = a.tab;
    const float2 *x = (const float2 *)a.rx + (size_t)b * a.rx_stride;
    const int tid = rx_tid();
    const bool leaving = S->bpf_grid != 0;     // leaving the grid at this call: memory = the 102 baseband samples before it, phase = the chain's value at this block boundary
    const float2 ph = leaving ? ((const float2 *)a.bpf_chain)[(size_t)b * a.chain_stride + 1 + calls0] : S->bpf_phase;
    const int nin0 = S->nin0;
    BpfLds *pl = (BpfLds *)&sh->xm[0];
    const int wave = tid >> 6, lane = tid & 63;
    BpfTaps taps; bpf_load_taps(taps, a.bpf16, lane);
    auto mixed = [&](int j) { return cmul_nc(x[cons0 + j], cmul_nc(ph, ld2(tab->bpf_E, j))); };       // baseband sample j of this call
    float2 head = make_float2(0.0f, 0.0f), body[BPF_NQ];
    if (tid < 102) head = leaving ? rx2_bpf_mem(a, b, nin0, cons0 - 102 + tid) : make_float2(st->bpf.mem[tid][0], st->bpf.mem[tid][1]);
#pragma unroll
    for (int q = 0; q < BPF_NQ; q++) { const int j = tid + 256 * q; body[q] = mixed(min(j, nin - 1)); if (j >= nin) body[q] = make_float2(0.0f, 0.0f); }
    const float2 memv = mixed(nin - 102 + min(tid, 101));      // new memory = the last 102 of [memory | new] (nin >= 800: all of them new samples)
    const float unsc = bpf_stage_planes(pl, (unsigned *)&sh->redi[14], tid, head, body, 0);
    // The outputs go to the stream's slice of the pre-pass buffer (what rade_batch_rx_filtered shows) AND, through LDS, to the caller: the caller's threads
    // read samples other lanes produced, and a plain global load may hit the vector L1 line the previous call's first-touch loads left there (stale
    // pre-pass values) -- stores go through to L2 without refreshing it.  xm is free once every wavefront is done with the planes.
    f32x4 re[2], im[2];
    for (int u = 0; u < 2; u++) { const int tile = wave + (NT2 / 64) * u; if (tile < BPF_TILES(nin)) bpf_fir_tile(pl, taps, tile, lane, re[u], im[u]); }
    __syncthreads();
    for (int u = 0; u < 2; u++) {
        const int tile = wave + (NT2 / 64) * u;
        if (tile >= BPF_TILES(nin)) continue;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int i = 256 * tile + 16 * (lane & 15) + 4 * (lane >> 4) + r;
            if (i < nin) { const float2 y = cmul_nc(make_float2(re[u][r] * unsc, im[u][r] * unsc), cconj(cmul_nc(ph, ld2(tab->bpf_E, i)))); rxf[cons0 + i] = y; sh->xm[i] = y; }
        }
    }
    __syncthreads();
    if (tid < 102) { st->bpf.mem[tid][0] = memv.x; st->bpf.mem[tid][1] = memv.y; }
    if (tid == 0) { S->bpf_phase = cmul_nc(ph, ld2(tab->bpf_E, nin - 1)); S->bpf_grid = 0; }
    __syncthreads();
}

// ---- the stand-alone kernels' view of their arguments (k_bpf_chain, k_bpf_fir, k_bpf_advance: rade_rx.hip) ----
__device__ __forceinline__ rd_bpf_state *bpf_state_of(const rd_bpf_args &a, int b) { return (rd_bpf_state *)((char *)a.state + (size_t)b * a.state_stride); }
__device__ __forceinline__ int bpf_len0_of(const rd_bpf_args &a, int b) { return a.len0 ? *(const int *)((const char *)a.len0 + (size_t)b * a.len0_stride) : a.len0_const; }
__device__ __forceinline__ int bpf_avail_of(const rd_bpf_args &a, int b) { return a.avail ? a.avail[b] : a.avail_const; }
// baseband sample q >= 0 of an invocation: x[q] times the phase of its block
__device__ __forceinline__ float2 bpf_baseband(const float2 *x, const float2 *chain, const rd_tables *tab, int nin0, int q)
{
    const int k = q < nin0 ? 0 : 1 + (q - nin0) / RD_NMF, sk = k ? nin0 + (k - 1) * RD_NMF : 0;
    return cmul_nc(x[q], cmul_nc(chain[1 + k], ld2(tab->bpf_E, q - sk)));
}
