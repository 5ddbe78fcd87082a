// xq_td_delta.inc.h — the text of td_delta_kernel, included by xq_td.hip.h once per TD loss (inside namespace xq; see there).  The includer
// defines XQ_TD_DELTA_KERNEL (the kernel's name), XQ_TD_DELTA_LOSS_PARAM (what the loss adds behind the last parameter, or nothing) and
// XQ_TD_DELTA_LOSS (the declaration of the loss object L).  A kernel per loss from ONE text, and not one inlined body under two kernels: the
// squared kernel keeps its name (profiles and cn_chess_ai_amd/workmodel.py know it by that) and, being the same function as before, its
// instructions — a body inlined into a wrapper compiles to other register assignments and another order of the argument loads.
// The rule itself is xq_td.hip.h's; called here: td_fold_max, first_max_take, td_target, td_output_delta, td_top_delta, td_record_store, per_priority_store.
__global__ __launch_bounds__(256) void XQ_TD_DELTA_KERNEL(int n, SlotSrc src,
                                                          const int32_t* __restrict__ action_to, const float* __restrict__ reward,
                                                          const uint8_t* __restrict__ done, const float* __restrict__ a_last, int H,
                                                          const float* __restrict__ w_out, const float* __restrict__ b_out,
                                                          const float* __restrict__ partial, int n_partial, float gamma,
                                                          const float* __restrict__ view, long long view_ld, int view_kmax,
                                                          float* __restrict__ dtop, float* __restrict__ dsc, int32_t* __restrict__ act,
                                                          float* __restrict__ qsa, float* __restrict__ yv, float* __restrict__ lossv,
                                                          TdExtra X XQ_TD_DELTA_LOSS_PARAM) {
    XQ_TD_DELTA_LOSS;
    const int wid = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const int b = (int)blockIdx.x * 4 + wid;
    if (b >= n) return;
    const int s = slot_of(src, b);
    const int a = action_to[s];
    const bool live = a >= 0 && a < 96;
    float delta = 0.f, q = 0.f, y = 0.f;
    const float* ar = a_last + (long long)b * H;
    if (H == 256 && !X.wout_bf && !X.double_dqn && n_partial <= 4) {
        // fp32 net, 256-wide last hidden layer, no arg-max: every load that depends only on (b, s, a) is
        // issued up front as one 16-byte load per lane — the general path below is a chain of five dependent memory round trips
        const int ac = live ? a : 0;
        const float4 av = *reinterpret_cast<const float4*>(ar + lane * 4);
        const float4 wv = *reinterpret_cast<const float4*>(w_out + (long long)ac * 256 + lane * 4);
        const bool has_view = live && a < view_kmax;
        const float4 vv = has_view ? *reinterpret_cast<const float4*>(view + (long long)a * view_ld + lane * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float zm = td_fold_max(partial, n, b, n_partial);
        const float bo = b_out[ac], r = reward[s];
        const bool dn = done[s] != 0;
        const float isw = X.is_w ? X.is_w[b] / X.is_wmax[0] : 1.f;
        float z = (av.x * wv.x + av.y * wv.y) + (av.z * wv.z + av.w * wv.w);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) z += __shfl_xor(z, off, 64);
        if (live) {
            q = tanhf(z + bo);
            y = td_target(r, dn, gamma, zm);
            delta = td_output_delta(L, q, y, isw);
        }
        *reinterpret_cast<float4*>(dtop + (long long)b * 256 + lane * 4) = td_top_delta(has_view, delta, vv, av);
    } else if (H == 512 && !X.wout_bf && !X.double_dqn && n_partial <= 4) {
        // fp32 net, 512-wide last hidden layer (BASELINE configs[3]): the 256-wide path with two 16-byte pieces per lane and row
        // (columns 4 lane + 256 v); per-lane partial = piece 0 + piece 1, then the same shuffle tree
        const int ac = live ? a : 0;
        const bool has_view = live && a < view_kmax;
        float4 av[2], wv[2], vv[2];
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            av[v] = *reinterpret_cast<const float4*>(ar + v * 256 + lane * 4);
            wv[v] = *reinterpret_cast<const float4*>(w_out + (long long)ac * 512 + v * 256 + lane * 4);
            vv[v] = has_view ? *reinterpret_cast<const float4*>(view + (long long)a * view_ld + v * 256 + lane * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const float zm = td_fold_max(partial, n, b, n_partial);
        const float bo = b_out[ac], r = reward[s];
        const bool dn = done[s] != 0;
        const float isw = X.is_w ? X.is_w[b] / X.is_wmax[0] : 1.f;
        float z = ((av[0].x * wv[0].x + av[0].y * wv[0].y) + (av[0].z * wv[0].z + av[0].w * wv[0].w)) +
                  ((av[1].x * wv[1].x + av[1].y * wv[1].y) + (av[1].z * wv[1].z + av[1].w * wv[1].w));
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) z += __shfl_xor(z, off, 64);
        if (live) {
            q = tanhf(z + bo);
            y = td_target(r, dn, gamma, zm);
            delta = td_output_delta(L, q, y, isw);
        }
#pragma unroll
        for (int v = 0; v < 2; ++v)
            *reinterpret_cast<float4*>(dtop + (long long)b * 512 + v * 256 + lane * 4) = td_top_delta(has_view, delta, vv[v], av[v]);
    } else if (H == 512 && X.wout_bf && n_partial <= 4 && (!X.double_dqn || X.wout_t_bf)) {
        // bf16 net, 512-wide last hidden layer (BASELINE configs[4]): the same idea — every load that depends only on (b, s, a) issued up
        // front, 8 columns per lane as 16-byte loads; Double DQN adds ONE dependent round trip (the target net's row of the arg-max)
        const int ac = live ? a : 0;
        const float* arp = ar + lane * 8;
        const float4 av0 = *reinterpret_cast<const float4*>(arp), av1 = *reinterpret_cast<const float4*>(arp + 4);
        const uint4 wq = *reinterpret_cast<const uint4*>(X.wout_bf + (long long)ac * 512 + lane * 8);
        const bool has_view = live && a < view_kmax;
        const float* vp = view + (long long)(has_view ? a : 0) * view_ld + lane * 8;
        float4 vv0 = *reinterpret_cast<const float4*>(vp), vv1 = *reinterpret_cast<const float4*>(vp + 4);
        float pm[4]; int pi[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            pm[t] = partial[(long long)min(t, n_partial - 1) * n + b];
            pi[t] = X.double_dqn ? X.partial_idx[(long long)min(t, n_partial - 1) * n + b] : 0;
        }
        uint4 atq = make_uint4(0u, 0u, 0u, 0u);
        if (X.double_dqn) atq = *reinterpret_cast<const uint4*>(X.alast_t_bf + (long long)b * 512 + lane * 8);
        const float bo = b_out[ac], r = reward[s];
        const bool dn = done[s] != 0;
        const float isw = X.is_w ? X.is_w[b] / X.is_wmax[0] : 1.f;
        auto lo = [](uint32_t x) { return __builtin_bit_cast(float, x << 16); };
        auto hi = [](uint32_t x) { return __builtin_bit_cast(float, x & 0xFFFF0000u); };
        float z = ((av0.x * lo(wq.x) + av0.y * hi(wq.x)) + (av0.z * lo(wq.y) + av0.w * hi(wq.y))) +
                  ((av1.x * lo(wq.z) + av1.y * hi(wq.z)) + (av1.z * lo(wq.w) + av1.w * hi(wq.w)));
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) z += __shfl_xor(z, off, 64);
        float zm = pm[0]; int zi = pi[0];
#pragma unroll
        for (int t = 1; t < 4; ++t) {
            if (X.double_dqn) first_max_take(zm, zi, pm[t], pi[t]);
            else zm = fmaxf(zm, pm[t]);
        }
        if (X.double_dqn) {          // value of the online net's greedy action on the TARGET net
            const int astar = (zi >= 0 && zi < X.nout) ? zi : 0;
            const uint4 tq = *reinterpret_cast<const uint4*>(X.wout_t_bf + (long long)astar * 512 + lane * 8);
            float zt = ((lo(atq.x) * lo(tq.x) + hi(atq.x) * hi(tq.x)) + (lo(atq.y) * lo(tq.y) + hi(atq.y) * hi(tq.y))) +
                       ((lo(atq.z) * lo(tq.z) + hi(atq.z) * hi(tq.z)) + (lo(atq.w) * lo(tq.w) + hi(atq.w) * hi(tq.w)));
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) zt += __shfl_xor(zt, off, 64);
            zm = zt + X.bout_t[astar];
        }
        if (live) {
            q = tanhf(z + bo);
            y = td_target(r, dn, gamma, zm);
            delta = td_output_delta(L, q, y, isw);
        }
        float4 o0 = make_float4(0.f, 0.f, 0.f, 0.f), o1 = o0;
        if (has_view) { o0 = td_top_delta(true, delta, vv0, av0); o1 = td_top_delta(true, delta, vv1, av1); }      // (one branch for both quads)
        float* dp = dtop + (long long)b * 512 + lane * 8;
        *reinterpret_cast<float4*>(dp) = o0;
        *reinterpret_cast<float4*>(dp + 4) = o1;
        if (X.dtop_bf)
            *reinterpret_cast<uint4*>(X.dtop_bf + (long long)b * 512 + lane * 8) =
                make_uint4((uint32_t)bf16_bits(o0.x) | ((uint32_t)bf16_bits(o0.y) << 16), (uint32_t)bf16_bits(o0.z) | ((uint32_t)bf16_bits(o0.w) << 16),
                           (uint32_t)bf16_bits(o1.x) | ((uint32_t)bf16_bits(o1.y) << 16), (uint32_t)bf16_bits(o1.z) | ((uint32_t)bf16_bits(o1.w) << 16));
    } else {
    if (live) {
        float z = 0.f;
        if (X.wout_bf) { const uint16_t* wr = X.wout_bf + (long long)a * H; for (int i = lane; i < H; i += 64) z += bf16_to_float(wr[i]) * ar[i]; }
        else { const float* wr = w_out + (long long)a * H; for (int i = lane; i < H; i += 64) z += wr[i] * ar[i]; }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) z += __shfl_xor(z, off, 64);
        z += b_out[a];
        float zm = partial[b];                         // max_k z_k(s'): the kReduceParts values colmax_reduce_kernel left per sample
        int zi = X.double_dqn ? X.partial_idx[b] : 0;
        for (int t = 1; t < n_partial; ++t) {
            const float v = partial[(long long)t * n + b];
            if (X.double_dqn) first_max_take(zm, zi, v, X.partial_idx[(long long)t * n + b]);
            else zm = fmaxf(zm, v);
        }
        if (X.double_dqn) {          // value of the online net's greedy action on the TARGET net
            const int astar = (zi >= 0 && zi < X.nout) ? zi : 0;
            float zt = 0.f;
            for (int i = lane; i < H; i += 64) {
                const float wv = X.wout_t_bf ? bf16_to_float(X.wout_t_bf[(long long)astar * H + i]) : X.wout_t[(long long)astar * H + i];
                const float av = X.alast_t_bf ? bf16_to_float(X.alast_t_bf[(long long)b * H + i]) : X.alast_t[(long long)b * H + i];
                zt += wv * av;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) zt += __shfl_xor(zt, off, 64);
            zm = zt + X.bout_t[astar];
        }
        q = tanhf(z);
        y = td_target(reward[s], done[s] != 0, gamma, zm);
        delta = td_output_delta(L, q, y, X.is_w ? X.is_w[b] / X.is_wmax[0] : 1.f);
    }
    float* drow = dtop + (long long)b * H;
    if (live && a < view_kmax) {
        const float* vr = view + (long long)a * view_ld;
        for (int i = lane; i < H; i += 64) {
            const float v = td_top_delta(delta, vr[i], ar[i]);
            drow[i] = v;
            if (X.dtop_bf) X.dtop_bf[(long long)b * H + i] = bf16_bits(v);
        }
    } else {
        for (int i = lane; i < H; i += 64) { drow[i] = 0.f; if (X.dtop_bf) X.dtop_bf[(long long)b * H + i] = 0; }
    }
    }
    if (lane == 0) {
        td_record_store(L, dsc, act, qsa, yv, lossv, b, live, a, delta, q, y);
        if (X.prio && live) per_priority_store(X.prio, X.pmax_live, s, q, y, X.per_eps, X.per_alpha);
    }
}
