// rade_rx_refine.h -- acquisition.refine (dsp.py:233-270): the fine timing / frequency search around (tmax, fmax), rx2_refine.  On sync entry (+-10 Hz, 80
// frequencies) direct sums: per frequency the phasor recurrence x_{n+2} = 2 cos(2w) x_n - x_{n-2} feeds f64 matrix products (refine2_tile).  In sync (+-1 Hz,
// 20-21 frequencies) the correlation is expanded about the grid's centre frequency w_c: eight moments of the pilot-window products, weighted with
// ((n - 79.5) / 80)^m e^{-j w_c n} (refine2_moments, f64 matrix products), then per grid frequency a polynomial in (w_k - w_c) 80 in registers.
// Part of rade_rx.hip's translation unit, behind rade_rx_search.h (block_argmax2).
// Members of RxShared2 it owns: rq, rzc, rph, rrot, ral (in-sync constants, prepared one call ahead by refine2_tables_sync), xm (the two windows as doubles),
// pd (pilot replica, loaded by the caller), rmom, mtot (in sync), rtw, rrot80, rt80, dtr (sync entry).
__device__ __forceinline__ f64x4 refine2_tile(const RxShared2 *sh, int mt, int frame, int s0, int ns, int nf, int nt, int lane)
{
    const int i = lane & 15, kk = lane >> 4, c = kk & 1, n0 = kk >> 1;
    const int row = 16 * mt + i, fi = row >> 1, cp = row & 1;
    const bool rv = fi < nf;
    const double2 z1 = sh->rtw[rv ? fi : 0];
    double2 cur = s0 ? sh->rt80[rv ? fi : 0] : make_double2(1.0, 0.0);
    if (n0) cur = make_double2(cur.x * z1.x - cur.y * z1.y, cur.x * z1.y + cur.y * z1.x);
    const double c2r = z1.x * z1.x - z1.y * z1.y, c2i = 2.0 * z1.x * z1.y;
    const double2 prv = make_double2(cur.x * c2r + cur.y * c2i, cur.y * c2r - cur.x * c2i);
    double xc = cp == c ? cur.x : (cp == 0 ? -cur.y : cur.y), xp = cp == c ? prv.x : (cp == 0 ? -prv.y : prv.y);
    if (!rv) { xc = 0.0; xp = 0.0; }
    const double k2 = 2.0 * c2r;
    const double *xw = (const double *)&sh->xm[0] + 4 * (frame * 176 + (i < nt ? i : 0) + 2 * s0 + n0) + 2 * c;
    const double2 *pp = &sh->pd[2 * s0 + n0];
    f64x4 acc0 = { 0.0, 0.0, 0.0, 0.0 }, acc1 = acc0;
    double2 pn[4]; double a1[4], a2[4];
#pragma unroll
    for (int u = 0; u < 4; u++) { pn[u] = pp[2 * u]; a1[u] = xw[8 * u]; a2[u] = xw[8 * u + 1]; }
#pragma unroll 1
    for (int s = 0; s < ns; s += 4) {
        double b[4];
#pragma unroll
        for (int u = 0; u < 4; u++) b[u] = pn[u].x * a1[u];
#pragma unroll
        for (int u = 0; u < 4; u++) b[u] = fma(pn[u].y, a2[u], b[u]);
        __builtin_amdgcn_sched_barrier(0);
        const int sn = s + 4 < ns ? s + 4 : s;
#pragma unroll
        for (int u = 0; u < 4; u++) { pn[u] = pp[2 * (sn + u)]; a1[u] = xw[8 * (sn + u)]; a2[u] = xw[8 * (sn + u) + 1]; }
        __builtin_amdgcn_sched_barrier(0);
        const double x1 = fma(k2, xc, -xp), x2 = fma(k2, x1, -xc), x3 = fma(k2, x2, -x1);
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(xc, b[0], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(x1, b[1], acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(x2, b[2], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(x3, b[3], acc1, 0, 0, 0);
        xp = x3; xc = fma(k2, x3, -x2);
        __builtin_amdgcn_sched_barrier(0);
    }
    return acc0 + acc1;
}
__device__ __forceinline__ void refine2_tables(RxShared2 *sh, int k, double fstart, double fstop, double fstep)
{
    const int nf = (int)ceil((fstop - fstart) / fstep);
    const double delta = (fstart + fstep) - fstart;
    if (k < 0 || k >= 3 * nf) return;
    const int which = k / nf, fi = k - which * nf;
    const double w = 2.0 * PI_D * dgrid_nc(fstart, fi, delta) / 8000.0;
    const double arg = which == 0 ? -w : (which == 1 ? -w * RD_NMF : -w * 80.0);
    double sn, cs; sincos(arg, &sn, &cs);
    double2 *dstp = which == 0 ? sh->rtw : (which == 1 ? sh->rrot80 : sh->rt80);
    dstp[fi] = make_double2(cs, sn);
}
__device__ __forceinline__ void refine2_tables_sync(RxShared2 *sh, int k, double fstart, double fstop, double fstep)
{
    const int nf = (int)ceil((fstop - fstart) / fstep);
    const double delta = (fstart + fstep) - fstart;
    const double wc = 0.5 * (2.0 * PI_D * fstart / 8000.0 + 2.0 * PI_D * dgrid_nc(fstart, nf - 1, delta) / 8000.0);
    if (k < 0 || k > 52) return;
    const int kf = k < 24 ? k : k - 24;
    if (k < 48 && kf >= nf) return;
    const double w = 2.0 * PI_D * dgrid_nc(fstart, kf, delta) / 8000.0, dw = w - wc;
    const double arg = k < 24 ? -w * RD_NMF : (k < 48 ? -dw * 79.5 : (k < 52 ? -wc * 40.0 * (k - 48) : -wc));
    double sn, cs; sincos(arg, &sn, &cs);
    const double2 v = make_double2(cs, sn);
    if (k < 24) sh->rrot[k] = v;
    else if (k < 48) { sh->rph[kf] = v; sh->ral[kf] = dw * 80.0; }
    else if (k < 52) sh->rq[k - 48] = v;
    else sh->rzc = v;
}
// moments of one quarter q of the samples (20 matrix instructions), added onto acc0 / acc1; the powers ((n - 79.5) / 80)^m come from L2
__device__ __forceinline__ void refine2_moments(const RxShared2 *sh, const double *vmg, int frame, int q, int nt, int lane, f64x4 &acc0, f64x4 &acc1)
{
    const int i = lane & 15, kk = lane >> 4, c = kk & 1, n0 = kk >> 1;
    const int m = i >> 1, cp = i & 1, s0 = 20 * q;
    const double2 z1 = sh->rzc;
    double2 cur = sh->rq[q];
    if (n0) cur = make_double2(cur.x * z1.x - cur.y * z1.y, cur.x * z1.y + cur.y * z1.x);
    const double c2r = z1.x * z1.x - z1.y * z1.y, c2i = 2.0 * z1.x * z1.y;
    const double2 prv = make_double2(cur.x * c2r + cur.y * c2i, cur.y * c2r - cur.x * c2i);
    double xc = cp == c ? cur.x : (cp == 0 ? -cur.y : cur.y), xp = cp == c ? prv.x : (cp == 0 ? -prv.y : prv.y);
    const double k2 = 2.0 * c2r;
    const double *xw = (const double *)&sh->xm[0] + 4 * (frame * 176 + (i < nt ? i : 0) + 2 * s0 + n0) + 2 * c;
    const double2 *pp = &sh->pd[2 * s0 + n0];
    // (an explicit global pointer: rx2_refine is a real function, its `vmg` a generic pointer, and the 20 loads below were flat loads, which count on the
    // LDS wait counter too; as global loads they do not -- measured: no change in the cycles per call, the batch is issued far enough ahead either way)
    const __attribute__((address_space(1))) double *vp = (const __attribute__((address_space(1))) double *)vmg + m * RD_M + 2 * s0 + n0;
    double vall[20];                                            // this lane's 20 powers of the quarter: one batch of loads ahead of the loop
#pragma unroll
    for (int u = 0; u < 20; u++) vall[u] = vp[2 * u];
    double2 pn[4]; double a1[4], a2[4];
#pragma unroll
    for (int u = 0; u < 4; u++) { pn[u] = pp[2 * u]; a1[u] = xw[8 * u]; a2[u] = xw[8 * u + 1]; }
#pragma unroll
    for (int s = 0; s < 20; s += 4) {
        double b[4];
#pragma unroll
        for (int u = 0; u < 4; u++) b[u] = pn[u].x * a1[u];
#pragma unroll
        for (int u = 0; u < 4; u++) b[u] = fma(pn[u].y, a2[u], b[u]);
        __builtin_amdgcn_sched_barrier(0);
        const int sn = s + 4 < 20 ? s + 4 : s;
#pragma unroll
        for (int u = 0; u < 4; u++) { pn[u] = pp[2 * (sn + u)]; a1[u] = xw[8 * (sn + u)]; a2[u] = xw[8 * (sn + u) + 1]; }
        __builtin_amdgcn_sched_barrier(0);
        const double x1 = fma(k2, xc, -xp), x2 = fma(k2, x1, -xc), x3 = fma(k2, x2, -x1);
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(xc * vall[s], b[0], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(x1 * vall[s + 1], b[1], acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(x2 * vall[s + 2], b[2], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(x3 * vall[s + 3], b[3], acc1, 0, 0, 0);
        xp = x3; xc = fma(k2, x3, -x2);
        __builtin_amdgcn_sched_barrier(0);
    }
}

__device__ void rx2_refine(RxShared2 *sh, const double *vmg, int *tmax, double *fmax, int t0, int nt, double fstart, double fstop, double fstep, bool in_sync)
{
    const int tid = rx_tid(), lane = tid & 63, wave = tid >> 6;
    const int nf = (int)ceil((fstop - fstart) / fstep);
    const double delta = (fstart + fstep) - fstart;
    const int ntasks = ((2 * nf + 15) >> 4) * 2;
    const int i = lane & 15, kk = lane >> 4;
    PH2_T0();
    if (!in_sync) refine2_tables(sh, tid, fstart, fstop, fstep);
    for (int j = tid; j < 2 * 176; j += NT2) {                            // the two windows as doubles: (xr, xi, xi, -xr)
        const int frame = j / 176, k = j - frame * 176;
        const float2 x = sh->rxb[min(t0 + frame * RD_NMF + k, RD_RXBUF - 1)];
        double *d = (double *)&sh->xm[0] + 4 * j;
        d[0] = (double)x.x; d[1] = (double)x.y; d[2] = (double)x.y; d[3] = -(double)x.x;
    }
    __syncthreads();
    PH2(27);
    float best = -1.0f; int bf = 0x7fffffff, bt = 0x7fffffff;
    if (in_sync) {
        // wavefront w = (half w >> 1 of the samples, frame w & 1): the two quarters of its half accumulate into the same tile
        {
            f64x4 a0 = { 0.0, 0.0, 0.0, 0.0 }, a1 = a0;
            refine2_moments(sh, vmg, wave & 1, 2 * (wave >> 1), nt, lane, a0, a1);
            refine2_moments(sh, vmg, wave & 1, 2 * (wave >> 1) + 1, nt, lane, a0, a1);
            const f64x4 part = a0 + a1;
#pragma unroll
            for (int r = 0; r < 4; r++) sh->rmom[wave >> 1][wave & 1][lane][r] = part[r];
        }
        __syncthreads();
        PH2(28);
        for (int o = tid; o < 2 * 64 * 4; o += NT2) {                     // C layout (f64 16x16x4): col = lane & 15 (t), row = (lane >> 4) + 4 * reg
            const int frame = o >> 8, l = (o >> 2) & 63, r = o & 3;
            sh->mtot[frame][(l >> 4) + 4 * r][l & 15] = sh->rmom[0][frame][l][r] + sh->rmom[1][frame][l][r];
        }
        __syncthreads();
        PH2(29);
        for (int o = tid; o < nf * 16; o += NT2) {
            const int fo = o >> 4, t = o & 15;
            if (t >= nt) continue;
            const double al = sh->ral[fo];
            const double2 ph = sh->rph[fo], rt = sh->rrot[fo];
            float2 d12[2];
#pragma unroll
            for (int frame = 0; frame < 2; frame++) {
                double re = 0.0, im = 0.0, cm = 1.0;
#pragma unroll
                for (int mq = 0; mq < 8; mq++) {
                    const double mr = sh->mtot[frame][2 * mq][t], mi = sh->mtot[frame][2 * mq + 1][t];
                    if ((mq & 3) == 0) { re = fma(cm, mr, re); im = fma(cm, mi, im); }
                    else if ((mq & 3) == 1) { re = fma(cm, mi, re); im = fma(-cm, mr, im); }
                    else if ((mq & 3) == 2) { re = fma(-cm, mr, re); im = fma(-cm, mi, im); }
                    else { re = fma(-cm, mi, re); im = fma(cm, mr, im); }
                    cm = cm * al * (1.0 / (double)(mq + 1));
                }
                double xr = re * ph.x - im * ph.y, xi = re * ph.y + im * ph.x;
                if (frame == 1) { const double tr = xr * rt.x - xi * rt.y; xi = xr * rt.y + xi * rt.x; xr = tr; }
                d12[frame] = make_float2((float)xr, (float)xi);
            }
            const float v = hypotf(d12[0].x + d12[1].x, d12[0].y + d12[1].y);
            if (v > best || (v == best && (fo < bf || (fo == bf && t < bt)))) { best = v; bf = fo; bt = t; }
        }
    } else {
        auto finish = [&](const f64x4 &acc, int mt, int frame) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const double mine = acc[r], other = __shfl_xor(mine, 16);
                if ((kk & 1) == 0) {
                    const int fo = 8 * mt + (kk >> 1) + 2 * r;
                    double re = mine, im = other;
                    if (frame == 1 && fo < nf) {
                        const double2 rt = sh->rrot80[fo];
                        const double tr = re * rt.x - im * rt.y; im = re * rt.y + im * rt.x; re = tr;
                    }
                    if (fo < nf && i < nt) sh->dtr[(frame * nf + fo) * 16 + i] = make_float2((float)re, (float)im);
                }
            }
        };
        for (int task = wave; task < ntasks; task += NW2) finish(refine2_tile(sh, task >> 1, task & 1, 0, 80, nf, nt, lane), task >> 1, task & 1);
        __syncthreads();
        for (int task = tid; task < nf * nt; task += NT2) {
            const int fi = task / nt, ti = task - fi * nt;
            const float2 a = sh->dtr[fi * 16 + ti], b = sh->dtr[(nf + fi) * 16 + ti];
            const float v = hypotf(a.x + b.x, a.y + b.y);
            if (v > best || (v == best && (fi < bf || (fi == bf && ti < bt)))) { best = v; bf = fi; bt = ti; }
        }
    }
    PH2(30);
    block_argmax2(sh, best, bf, bt);
    PH2(31);
    if (best > 0.0f) { *tmax = t0 + bt; *fmax = dgrid_nc(fstart, bf, delta); }      // (two roundings, like np.arange's elements: rade_devutil.h)
}
