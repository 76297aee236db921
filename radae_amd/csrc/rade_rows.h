// rade_rows.h -- small data-movement kernels around the GEMMs and their launch shims; part of rade_kernels.hip (see its inventory).
// Replaces: the feature packing of radae_txe.py:114-121 (k_enc_pack); the torch.cat / F.pad bookkeeping of the layer stack (k_pad_rows: GEMM inputs zero-padded
// to K % 8 == 0; k_carry_rows: the conv history rows carried to the next chunk).  Needs RD_ENC_IN (rade_dev.h) only.
__global__ void k_enc_pack(const float *features, float *xin, int B, int T)
{   // model19 only: 4 x (20 features + aux symbol -1) padded 84 -> 88
    __builtin_amdgcn_s_setprio(3);
    const long n = (long)B * T * RD_ENC_IN;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % RD_ENC_IN); const long bt = i / RD_ENC_IN;
        float v = 0.0f;
        if (c < RM_FEAT_AUX) { const int fr = c / (RM_NFEAT + 1), j = c - fr * (RM_NFEAT + 1); v = j < RM_NFEAT ? features[(bt * RM_STEP_FRAMES + fr) * RM_FILE_FRAME + j] : -1.0f; }
        xin[i] = v;
    }
}
extern "C" int rd_launch_enc_pack(const float *features, float *xin, int B, int T, rd_stream_t s)
{
    const long n = (long)B * T * RD_ENC_IN; if (n <= 0) return 0;
    int grid = (int)((n + 255) / 256); if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(k_enc_pack, dim3(grid), dim3(256), 0, (hipStream_t)s, features, xin, B, T);
    return (int)hipGetLastError();
}

// dense rows [R][K] -> [R][Kpad] with zero fill (GEMM K must be a multiple of 8)
__global__ void k_pad_rows(const float *src, float *dst, long R, int K, int Kpad)
{
    const long n = R * Kpad;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % Kpad); const long r = i / Kpad;
        dst[i] = c < K ? src[r * K + c] : 0.0f;
    }
}
extern "C" int rd_launch_pad_rows(const float *src, float *dst, long R, int K, int Kpad, rd_stream_t s)
{
    const long n = R * Kpad; if (n <= 0) return 0;
    int grid = (int)((n + 255) / 256); if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(k_pad_rows, dim3(grid), dim3(256), 0, (hipStream_t)s, src, dst, R, K, Kpad);
    return (int)hipGetLastError();
}

// x is [B][nhist+Tcap][W]; copy rows [Tb, Tb+nhist) -> [0, nhist)  (Tb = n_rows[b] or T).  Source and
// destination overlap when Tb < nhist, so every thread reads all its elements before any write.
__global__ __launch_bounds__(256) void k_carry_rows(float *x, int Tcap, int W, int nhist, int T, const int *n_rows)
{
    __builtin_amdgcn_s_setprio(3);
    const int b = blockIdx.x;
    const int Tb = n_rows ? n_rows[b] : T;
    if (Tb <= 0) return;
    float *base = x + (size_t)b * (nhist + Tcap) * W;
    const int n = nhist * W;       // <= 2048
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; q++) { const int i = threadIdx.x + q * 256; v[q] = i < n ? base[(size_t)Tb * W + i] : 0.0f; }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; q++) { const int i = threadIdx.x + q * 256; if (i < n) base[i] = v[q]; }
}
extern "C" int rd_launch_carry_rows(float *x, int B, int Tcap, int W, int nhist, int T, const int *n_rows, rd_stream_t s)
{
    if (B <= 0) return 0;
    if (nhist < 1 || (long)nhist * W > 2048) return -1;       // k_carry_rows holds the history in 8 registers x 256 threads
    hipLaunchKernelGGL(k_carry_rows, dim3(B), dim3(256), 0, (hipStream_t)s, x, Tcap, W, nhist, T, n_rows);
    return (int)hipGetLastError();
}
