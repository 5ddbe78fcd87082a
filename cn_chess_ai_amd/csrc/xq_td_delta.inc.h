// xq_td_delta.inc.h — the text of td_delta_kernel, included by xq_tail.hip.h once per TD loss (inside namespace xq; see there).  The includer
// defines XQ_TD_DELTA_KERNEL (the kernel's name), XQ_TD_DELTA_LOSS_PARAM (what the loss adds behind the last parameter, or nothing) and
// XQ_TD_DELTA_LOSS (the declaration of the loss object L).  A kernel per loss from ONE text, and not one inlined body under two kernels: the
// squared kernel keeps its name (profiles and cn_chess_ai_amd/workmodel.py know it by that) and, being the same function as before, its
// instructions — a body inlined into a wrapper compiles to other register assignments and another order of the argument loads.
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
        float zm = partial[b];                         // the (up to kReduceParts) maxima left per sample
#pragma unroll
        for (int t = 1; t < 4; ++t) zm = fmaxf(zm, partial[(long long)min(t, n_partial - 1) * n + b]);
        const float bo = b_out[ac], r = reward[s];
        const bool dn = done[s] != 0;
        const float isw = X.is_w ? X.is_w[b] / X.is_wmax[0] : 1.f;
        float z = (av.x * wv.x + av.y * wv.y) + (av.z * wv.z + av.w * wv.w);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) z += __shfl_xor(z, off, 64);
        if (live) {
            q = tanhf(z + bo);
            y = dn ? r : r + gamma * tanhf(zm);
            delta = L.err(q - y) * td_dtanh(q) * isw;
        }
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (has_view) {
            o.x = delta * vv.x * (1.f - av.x * av.x); o.y = delta * vv.y * (1.f - av.y * av.y);
            o.z = delta * vv.z * (1.f - av.z * av.z); o.w = delta * vv.w * (1.f - av.w * av.w);
        }
        *reinterpret_cast<float4*>(dtop + (long long)b * 256 + lane * 4) = o;
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
        float zm = partial[b];
#pragma unroll
        for (int t = 1; t < 4; ++t) zm = fmaxf(zm, partial[(long long)min(t, n_partial - 1) * n + b]);
        const float bo = b_out[ac], r = reward[s];
        const bool dn = done[s] != 0;
        const float isw = X.is_w ? X.is_w[b] / X.is_wmax[0] : 1.f;
        float z = ((av[0].x * wv[0].x + av[0].y * wv[0].y) + (av[0].z * wv[0].z + av[0].w * wv[0].w)) +
                  ((av[1].x * wv[1].x + av[1].y * wv[1].y) + (av[1].z * wv[1].z + av[1].w * wv[1].w));
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) z += __shfl_xor(z, off, 64);
        if (live) {
            q = tanhf(z + bo);
            y = dn ? r : r + gamma * tanhf(zm);
            delta = L.err(q - y) * td_dtanh(q) * isw;
        }
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            if (has_view) {
                o.x = delta * vv[v].x * (1.f - av[v].x * av[v].x); o.y = delta * vv[v].y * (1.f - av[v].y * av[v].y);
                o.z = delta * vv[v].z * (1.f - av[v].z * av[v].z); o.w = delta * vv[v].w * (1.f - av[v].w * av[v].w);
            }
            *reinterpret_cast<float4*>(dtop + (long long)b * 512 + v * 256 + lane * 4) = o;
        }
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
            if (X.double_dqn) { if (pm[t] > zm || (pm[t] == zm && pi[t] < zi)) { zm = pm[t]; zi = pi[t]; } }
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
            y = dn ? r : r + gamma * tanhf(zm);
            delta = L.err(q - y) * td_dtanh(q) * isw;
        }
        float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (has_view) {
            o[0] = delta * vv0.x * (1.f - av0.x * av0.x); o[1] = delta * vv0.y * (1.f - av0.y * av0.y);
            o[2] = delta * vv0.z * (1.f - av0.z * av0.z); o[3] = delta * vv0.w * (1.f - av0.w * av0.w);
            o[4] = delta * vv1.x * (1.f - av1.x * av1.x); o[5] = delta * vv1.y * (1.f - av1.y * av1.y);
            o[6] = delta * vv1.z * (1.f - av1.z * av1.z); o[7] = delta * vv1.w * (1.f - av1.w * av1.w);
        }
        float* dp = dtop + (long long)b * 512 + lane * 8;
        *reinterpret_cast<float4*>(dp) = make_float4(o[0], o[1], o[2], o[3]);
        *reinterpret_cast<float4*>(dp + 4) = make_float4(o[4], o[5], o[6], o[7]);
        if (X.dtop_bf)
            *reinterpret_cast<uint4*>(X.dtop_bf + (long long)b * 512 + lane * 8) =
                make_uint4((uint32_t)bf16_bits(o[0]) | ((uint32_t)bf16_bits(o[1]) << 16), (uint32_t)bf16_bits(o[2]) | ((uint32_t)bf16_bits(o[3]) << 16),
                           (uint32_t)bf16_bits(o[4]) | ((uint32_t)bf16_bits(o[5]) << 16), (uint32_t)bf16_bits(o[6]) | ((uint32_t)bf16_bits(o[7]) << 16));
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
            if (X.double_dqn) {
                const int vi = X.partial_idx[(long long)t * n + b];
                if (v > zm || (v == zm && vi < zi)) { zm = v; zi = vi; }
            } else zm = fmaxf(zm, v);
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
        const float r = reward[s];
        y = done[s] ? r : r + gamma * tanhf(zm);       // max_k tanh(z_k) = tanh(max_k z_k)
        delta = L.err(q - y) * td_dtanh(q);          // (a - target) * (1 - tanh(z)^2), the error through the loss
        if (X.is_w) delta *= X.is_w[b] / X.is_wmax[0];
    }
    float* drow = dtop + (long long)b * H;
    if (live && a < view_kmax) {
        const float* vr = view + (long long)a * view_ld;
        for (int i = lane; i < H; i += 64) {
            const float h = ar[i];
            const float v = delta * vr[i] * (1.f - h * h);
            drow[i] = v;
            if (X.dtop_bf) X.dtop_bf[(long long)b * H + i] = bf16_bits(v);
        }
    } else {
        for (int i = lane; i < H; i += 64) { drow[i] = 0.f; if (X.dtop_bf) X.dtop_bf[(long long)b * H + i] = 0; }
    }
    }
    if (lane == 0) {
        dsc[b] = delta;
        act[b] = live ? a : -1;
        qsa[b] = q; yv[b] = y;
        lossv[b] = live ? L.loss(q - y) : 0.f;
        if (X.prio && live) {
            const float p = powf(fabsf(q - y) + X.per_eps, X.per_alpha);
            X.prio[s] = p;
            // the running maximum rarely moves once training is under way: test first, so that 16 K waves do not queue on one address
            // (positive floats order like their bit patterns; a maximum is order-independent, hence still deterministic)
            if (__float_as_uint(p) > __hip_atomic_load(X.pmax_live, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                atomicMax(X.pmax_live, __float_as_uint(p));
        }
    }
}
