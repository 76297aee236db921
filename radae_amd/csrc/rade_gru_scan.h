// rade_gru_scan.h -- the GRU recurrence over a chunk and its launch shim; part of rade_kernels.hip (see its inventory).
// Replaces: the time loop of torch.nn.GRU inside CoreEncoder / CoreDecoder (radae_base.py:97-108); the input projections W_ih x are GEMMs (rade_gemm.h).
// Needs rd_scan_args, RD_DEC_ROWS_MAX, RD_EF_TILE (rade_dev.h); quad_dpp, gate_sigmoid, gate_tanh, clamp1, split16_act (rade_devutil.h).
// GRU recurrence (the only serial part of a layer): h_t = f(gi_t, W_hh h_{t-1}), one workgroup per stream.
// Four adjacent lanes own hidden unit j; lane part p holds the r/z/n rows of W_hh for k in [p*H/4, (p+1)*H/4)
// in VGPRs, partial dot products meet through quad shuffles, every lane of the quad evaluates the gates
// (no divergence) and part 0 publishes h_j to LDS: one barrier per time step.
template <int H>
__global__ __launch_bounds__(4 * H) void k_gru_scan(rd_scan_args a)
{
    // a latency chain (one barrier per step, a handful of instructions between two of them) that shares its SIMDs with receiver wavefronts of other batches:
    // at the default priority every one of its instructions queues behind theirs (72 us per launch alone, 200 us in the pipelined bench); raised, the
    // recurrence runs close to its own latency and takes few issue slots from anybody (same-box A/B: +1.6 .. +3.3 % frames/s; the GEMM / modulator / channel
    // kernels, which are throughput-bound, gained nothing from the same treatment)
    __builtin_amdgcn_s_setprio(3);
    constexpr int KP = H / 4;                       // k range per lane
    __shared__ __attribute__((aligned(16))) float hs[2][H];   // double-buffered so one barrier per step suffices
    __shared__ int rst[RD_DEC_ROWS_MAX];            // reset flags are only used by the decoder rounds (T <= 384)
    const int b = blockIdx.x, tid = threadIdx.x, j = tid >> 2, p = tid & 3;
    float wr[KP], wz[KP], wn[KP];
    {
        const float *w0 = a.Whh + (size_t)j * H + p * KP;
#pragma unroll
        for (int k = 0; k < KP; k += 4) {
            const f32x4 v0 = *(const f32x4 *)(w0 + k), v1 = *(const f32x4 *)(w0 + (size_t)H * H + k), v2 = *(const f32x4 *)(w0 + (size_t)2 * H * H + k);
#pragma unroll
            for (int u = 0; u < 4; u++) { wr[k + u] = v0[u]; wz[k + u] = v1[u]; wn[k + u] = v2[u]; }
        }
    }
    const float br = a.bhh[j], bz = a.bhh[H + j], bn = a.bhh[2 * H + j];
    const int Tb = a.n_rows ? a.n_rows[b] : a.T;
    if (a.reset) for (int i = tid; i < a.T && i < RD_DEC_ROWS_MAX; i += blockDim.x) rst[i] = a.reset[b * a.reset_sb + i];
    float hj = a.h[(size_t)b * H + j];
    if (p == 0) hs[0][j] = hj;
    _Float16 *of = nullptr;                         // the batched encoder's fragment buffer (rade_enc.hip): unit j's slot in row 0 of the stream's history tile
    if (a.outf) { const int col = a.outf_col + j; of = (_Float16 *)a.outf + (size_t)b * a.outf_NQ * RD_EF_TILE + (col >> 4) * 1024 + ((col >> 3) & 1) * 256 + (col & 7); }
    const float *gi = a.gi + (size_t)b * a.gi_sb + (p < 3 ? p * H + j : j);   // lane part p < 3 fetches gate p of unit j
    // gi is fetched four steps at a time into TWO register sets that take turns: a set is refilled right after its block of steps and consumed a whole
    // block later, so the loads land in the registers they are used from.  (Rounds 1-3 had one set and a copy "next -> current" at the end of a block: the
    // compiler put the fresh loads and `s_waitcnt vmcnt(0)` in front of that copy -- a memory round trip exposed every four steps, a quarter of the step.)
    // Rows beyond Tb re-read the last row (never used): no branch around a load.
    float gA[4], gB[4];
    auto fetch = [&](float (&dst)[4], int t0) {
#pragma unroll
        for (int u = 0; u < 4; u++) dst[u] = gi[(size_t)min(t0 + u, max(Tb - 1, 0)) * a.gi_st];
    };
    // every load issued so far (W_hh rows, biases, state) completes here: left pending into the loop, the wait-count bookkeeping (one state per loop header,
    // merged over entry and back edge) makes the first step of every block wait for ALL outstanding loads
    __builtin_amdgcn_s_waitcnt(0x0F70);          // vmcnt(0)
    __builtin_amdgcn_sched_barrier(0);
    fetch(gA, 0); fetch(gB, 4);
    __syncthreads();
    int cur = 0;
    // fragment output (the batched encoder): a step's h leaves one step later -- the conversion to two binary16 planes and the two 2-byte stores are not on the
    // path between two barriers (on it they cost 40 ns per step: 0.39 -> 0.44 ms over the five scans of an encoder pass)
    float pend = 0.0f; int tpend = -1;
    auto store_frag = [&](int tp) {
        if (p == 0) {
            _Float16 *o = of + (size_t)(1 + (tp >> 5)) * RD_EF_TILE + (tp & 31) * 8;
            split16_act(clamp1(pend), o[0], o[512]);
        }
    };
    auto block = [&](const float (&gq)[4], int t0) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int t = t0 + u;
            if (t >= Tb) break;
            if (a.reset && rst[t]) {                       // uniform over the workgroup
                hj = 0.0f;
                __syncthreads();
                if (p == 0) hs[cur][j] = 0.0f;
                __syncthreads();
            }
            // this lane's quarter of the three dot products as packed FMAs (even / odd k in the two halves of an accumulator pair): 3 KP / 2 instructions
            // instead of 3 KP on the step's serial path
            // (the three dot products one after the other, each gate's exp2 / rcp started under the next product's multiply-adds: 0.472 against 0.414 ms over the five
            // scans of a pass -- two dependent accumulator chains per product instead of six independent ones; profiles/r05_ab_notes.txt)
            f32x2 ar = { 0.0f, 0.0f }, az = ar, an = ar;
            const float *hp = hs[cur] + p * KP;
#pragma unroll
            for (int k = 0; k < KP; k += 4) {
                const f32x4 hv = *(const f32x4 *)(hp + k);
                const f32x2 h0 = { hv[0], hv[1] }, h1 = { hv[2], hv[3] };
                ar = __builtin_elementwise_fma((f32x2){ wr[k], wr[k + 1] }, h0, ar); az = __builtin_elementwise_fma((f32x2){ wz[k], wz[k + 1] }, h0, az); an = __builtin_elementwise_fma((f32x2){ wn[k], wn[k + 1] }, h0, an);
                ar = __builtin_elementwise_fma((f32x2){ wr[k + 2], wr[k + 3] }, h1, ar); az = __builtin_elementwise_fma((f32x2){ wz[k + 2], wz[k + 3] }, h1, az); an = __builtin_elementwise_fma((f32x2){ wn[k + 2], wn[k + 3] }, h1, an);
            }
            if (of && tpend >= 0) store_frag(tpend);       // the previous step's output: independent of this step's chain, issued behind its multiply-adds
            float sr = ar[0] + ar[1], sz = az[0] + az[1], sn = an[0] + an[1];
            sr += quad_dpp<QUAD_XOR1>(sr); sz += quad_dpp<QUAD_XOR1>(sz); sn += quad_dpp<QUAD_XOR1>(sn);
            sr += quad_dpp<QUAD_XOR2>(sr); sz += quad_dpp<QUAD_XOR2>(sz); sn += quad_dpp<QUAD_XOR2>(sn);
            const float g0 = gq[u];
            const float gr = quad_dpp<QUAD_BC0>(g0), gz = quad_dpp<QUAD_BC1>(g0), gn = quad_dpp<QUAD_BC2>(g0);
            const float r = gate_sigmoid((sr + br) + gr);
            const float z = gate_sigmoid((sz + bz) + gz);
            const float n = gate_tanh(gn + (sn + bn) * r);
            hj = (hj - n) * z + n;
            if (p == 0) {
                hs[cur ^ 1][j] = hj;
                if (!of) a.out[(size_t)b * a.out_sb + (size_t)t * a.out_st + j] = clamp1(hj);
            }
            pend = hj; tpend = t;
            cur ^= 1;
            __syncthreads();
        }
    };
    for (int t0 = 0; t0 < Tb; t0 += 8) {
        block(gA, t0);
        fetch(gA, t0 + 8);
        block(gB, t0 + 4);
        fetch(gB, t0 + 12);
    }
    if (of && tpend >= 0) store_frag(tpend);
    if (p == 0) a.h[(size_t)b * H + j] = hj;
}

extern "C" int rd_launch_gru_scan(const rd_scan_args *a, rd_stream_t s)
{
    if (a->B <= 0) return 0;
    hipStream_t st = (hipStream_t)s;
    if (a->H == RM_ENC_H) hipLaunchKernelGGL(k_gru_scan<RM_ENC_H>, dim3(a->B), dim3(4 * RM_ENC_H), 0, st, *a);
    else if (a->H == RM_DEC_H) hipLaunchKernelGGL(k_gru_scan<RM_DEC_H>, dim3(a->B), dim3(4 * RM_DEC_H), 0, st, *a);
    else return -1;
    return (int)hipGetLastError();
}
