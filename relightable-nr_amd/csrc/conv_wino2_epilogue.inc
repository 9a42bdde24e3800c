// The F(2x2, 2x2) epilogue, written once and included at the end of conv_wino2_kernel<1> and conv_wino2p_kernel<2> (conv_wino2.inc,
// conv_wino2p.inc): Y = A^T M A per (tile, column), statistics, BatchNorm arrival, stores.
// It is a fragment of the kernel body, not a function: as a __forceinline__ function the compiler simplifies it on its own before
// inlining and both kernels came out slower (more scalar work, an extra spill in the transposed kernel's K loop; 0.8 % of the
// 16-view frame).  The including kernel provides: P, KIND, T (W2Tile), acc (floatx16[6], [plane nu][column half]), xi, l31, h,
// As (its dynamic LDS, dead halo by now) and CHUNK (floats per staged K block).  As holds the exchange rounds, the
// statistics scratch (a slot per wave) behind them.
{

    static_assert((2 * CHUNK > W2_XCHG ? 2 * CHUNK : W2_XCHG) % 2 == 0, "float64 scratch alignment");
    double* red = W2Stats::red(As + (2 * CHUNK > W2_XCHG ? 2 * CHUNK : W2_XCHG));
    constexpr int BNW = W2Kind<KIND>::BNW;
    const int tid = T.tid, lane = T.lane, n = T.n;
    // rr[g][half] = (r[b = 0], r[b = 1]) of this wave's plane row: r0 = M0 + M1, r1 = M1 - M2
    float2 rr[16][2];
#pragma unroll
    for (int g = 0; g < 16; g++)
#pragma unroll
        for (int nb = 0; nb < 2; nb++) {
            rr[g][nb].x = acc[0 + nb][g] + acc[2 + nb][g];
            rr[g][nb].y = acc[2 + nb][g] - acc[4 + nb][g];
        }
    // wave xi finishes register rows [G0, G1): Y0 = R0 + R1, Y1 = R1 - R2 over the plane rows of its group
    float2 y0v[6][2], y1v[6][2];        // [row][half]; waves 1, 2 use five rows
    float2* xb = reinterpret_cast<float2*>(As);             // [wave][<= 11 rows it does not finish][lane]
    const int wbase = T.wgrp * 3;
    auto finish = [&](auto F) {
        constexpr int f = decltype(F)::value;
        constexpr int G0[3] = {0, 6, 11}, G1[3] = {6, 11, 16};
#pragma unroll
        for (int nb = 0; nb < 2; nb++) {
            __syncthreads();        // round 0: every wave is done with the halo; round 1: with the previous exchange
            int k = 0;
#pragma unroll
            for (int g = 0; g < 16; g++) {
                if (g >= G0[f] && g < G1[f]) continue;
                xb[((wbase + f) * 11 + k) * 64 + lane] = rr[g][nb];
                k++;
            }
            __syncthreads();
#pragma unroll
            for (int g = G0[f]; g < G1[f]; g++) {
                float2 R[3];
#pragma unroll
                for (int o = 0; o < 3; o++) {
                    if (o == f) { R[o] = rr[g][nb]; continue; }
                    // position of row g among the rows wave o does not finish
                    const int ko = g < G0[o] ? g : g - (G1[o] - G0[o]);
                    R[o] = xb[((wbase + o) * 11 + ko) * 64 + lane];
                }
                y0v[g - G0[f]][nb] = make_float2(R[0].x + R[1].x, R[0].y + R[1].y);
                y1v[g - G0[f]][nb] = make_float2(R[1].x - R[2].x, R[1].y - R[2].y);
            }
        }
    };
    if (xi == 0) finish(std::integral_constant<int, 0>{});
    else if (xi == 1) finish(std::integral_constant<int, 1>{});
    else finish(std::integral_constant<int, 2>{});
    const int g0 = xi == 0 ? 0 : (xi == 1 ? 6 : 11), ng = xi == 0 ? 6 : 5;

    double s1[2] = {0.0, 0.0}, s2[2] = {0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 6; k++)
#pragma unroll
        for (int nb = 0; nb < 2; nb++) {
            if (k < ng) {
                const double a = y0v[k][nb].x, b = y0v[k][nb].y, c = y1v[k][nb].x, d = y1v[k][nb].y;
                s1[nb] += (a + b) + (c + d);
                s2[nb] += (a * a + b * b) + (c * c + d * d);
            }
        }
    const bool with_stats = P.stats != nullptr && P.splitk == 1;
    if (with_stats) {
#pragma unroll
        for (int nb = 0; nb < 2; nb++) {
            s1[nb] += __shfl_xor(s1[nb], 32, 64);
            s2[nb] += __shfl_xor(s2[nb], 32, 64);
            if (h == 0) {
                red[(T.wave * 64 + 32 * nb + l31) * 2 + 0] = s1[nb];
                red[(T.wave * 64 + 32 * nb + l31) * 2 + 1] = s2[nb];
            }
        }
        // KIND 2: all twelve waves hold the workgroup's 64 columns; KIND 1: the six waves w with ((w / 3) & 1) == tid / 64
        // hold column half tid / 64
        W2Stats::publish<BNW>(P, red, n, T.nt * BNW, tid,
                            [tid](int j) { return KIND == 1 ? (j / 3) * 6 + (tid >> 6) * 3 + j % 3 : j; });
    }
    BnArrival arr = {nullptr, 0u};
    const bool bn = with_stats && P.arrive;
    if (bn) arr = bn_arrive(P, n, tid);
    {
        // register row g = tile row g >> 2, tile column (g & 3) + 4 h; outputs (2 ty + e, 2 tx + f) of the tile.
        // ColumnStore's layout written out: through the struct the transposed kernel's K loop gains four 16-byte scratch accesses
        constexpr int XM = KIND == 2 ? 2 : 1;       // transposed conv: this parity class writes every other pixel
        const int Y00 = XM * (T.y0 + 8 * T.mb) + (KIND == 2 ? T.py : 0), X00 = XM * T.x0 + (KIND == 2 ? T.grp : 0);
        float* base = P.out + (size_t)T.z * P.slab_stride + (((size_t)n * P.OH + Y00) * P.OW + X00) * P.c_out_pad + T.n0;
        const __amdgpu_buffer_rsrc_t rsrc = buffer_rsrc(base);
        const unsigned cp4 = (unsigned)P.c_out_pad * 4u;
        unsigned voff[2];
#pragma unroll
        for (int nb = 0; nb < 2; nb++)
            voff[nb] = (T.n0 + 32 * nb + l31 < P.c_out_pad) ? (unsigned)(XM * 8 * h) * cp4 + (unsigned)(32 * nb + l31) * 4u : 0x7fffffffu;
#pragma unroll
        for (int k = 0; k < 6; k++) {
            if (k >= ng) continue;
            const int g = g0 + k;
            const int tyr = g >> 2, txr = g & 3;
#pragma unroll
            for (int e = 0; e < 2; e++)
#pragma unroll
                for (int f = 0; f < 2; f++)
#pragma unroll
                    for (int nb = 0; nb < 2; nb++) {
                        const unsigned soff = (unsigned)(XM * ((2 * tyr + e) * P.OW + 2 * txr + f)) * cp4;
                        const float2 yy = e ? y1v[k][nb] : y0v[k][nb];
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(f ? yy.y : yy.x), rsrc, (int)voff[nb], (int)soff, WINO_OUT_AUX);
                    }
        }
    }
    if (bn) bn_complete(P, arr, n, tid, W2Stats::flag(red));
}
