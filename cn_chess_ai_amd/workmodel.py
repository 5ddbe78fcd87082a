"""Algorithmic work of every kernel of the training step — FLOPs and COMPULSORY HBM bytes per launch.

Measurement support for bench.py's `roofline` / `roofline_chain` (no compute, no device access).  "Compulsory" = every distinct input
read once and every output written once at the sizes the kernel is launched with; re-reads served by L2 / the Infinity Cache (the
layer-0 gathers touch ~32 rows of W0^T per sample, the weight-gradient blocks re-read their operands per tile) are NOT counted —
rocprofv3's FETCH_SIZE / WRITE_SIZE (profiles/*_pmc_hbm_traffic.json) over these bytes is the waste ratio the judge asks for.

Names are the bracket names of xq_dqn_kernel_stats; "@select" = the same kernel in the self-play loop's select chain (collect
stream).  Per-LAUNCH figures: a kernel launched several times per step (td_tail_deltas of a 3-hidden-layer net, the select
chain with several plies per update) gets the mean over its launches of one step.
"""

NO = 8100            # outputs (90 x 90 actions, chessai.cpp:399-402)
STATE = 1260         # 90 x 14 one-hot inputs, never materialised
ENV_BYTES_PER_GAME = 2 * (48 + 16) + 360 + 105   # board+meta r/w, Q row, transition record

PEAK_F32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md: dense fp32 matrix peak
PEAK_BF16_MFMA_TFLOPS = 2500.0    # MI355X_MICROARCH.md: dense bf16 matrix peak (the 5 PF headline figure includes 2:1 sparsity)
PEAK_HBM_GBS = 8000.0             # MI355X_MICROARCH.md: HBM3E spec peak

# bracket name -> the kernel instance rocprofv3 prints for it: base name + template arguments, matched as a PREFIX of the printed name
# ("void xq::" stripped) so that a renamed kernel or a changed template argument fails the lookup instead of silently reading the figures
# of an older build (`td_tail_kernel<30u>` no longer matched `td_tail_kernel<30u, false>`).  Fixed names first; the
# configuration-dependent ones are in rocprof_kernel().
ROCPROF_NAMES = {
    "l0_forward_gather": "l0_forward_kernel<",            # <false> fp32 net, <true> bf16 net: one instance per configuration
    "l0_forward_gather@select": "l0_forward_kernel<",
    "td_target_delta": "td_delta_kernel(",
    "colmax_reduce": "colmax_reduce_kernel(",
    "sgd_apply": "sgd_segments_kernel(",
    "adam_apply": "adam_segments_kernel(",
    "grad_norm": "grad_norm_kernel(",
    "env_selfplay_step": "env_kernel<2>(",
    "target_sync_copy": "__amd_rocclr_copyBuffer",
    "l0_grad_segsum": "l0_grad_kernel(",
    "out_grad_segsum": "out_grad_kernel(",
    "bias_grad_colsum": "colsum_partial_kernel(",
    "nstep_assemble": "nstep_assemble_kernel(",
    "per_writeback": "per_writeback_kernel(",
    "mirror_stage": "mirror_stage_kernel(",
    "colour_swap_stage": "colour_swap_stage_kernel(",
    "mover_view_stage": "mover_view_stage_kernel(",
    "view_boards@select": "view_boards_kernel(",
    "legal_qmax": "legal_qmax_kernel(",
    "legal_side_stage": "legal_side_stage_kernel(",
    "gemm_legal_head": "gemm_f32_kernel<0, 0, 0, 1, 1, 0>(",
}
# td_tail_kernel<KINDS, L0MFMA>: KINDS = TAIL_DELTA 1 | TAIL_GRAD 2 | TAIL_OUT 4 | TAIL_COLSUM 8 | TAIL_L0 16 | TAIL_SEL 32 (xq_tail.hip.h)
TAIL_DELTAS, TAIL_DELTAS_SEL, TAIL_L0 = 7, 39, 30


def rocprof_kernel(name, layers, minibatch, td="online", bf16=False, l0_mfma=True, n_games=None):
    """The kernel instance(s) of a bracket name as rocprofv3 prints them (prefix after "void xq::"), or None when the bracket has no
    single kernel.  A list: several instances share the bracket (traffic = their mean)."""
    Hl, dbl, k = layers[-2], td == "double", len(layers) - 2
    mfma = l0_mfma and layers[1] % 64 == 0 and minibatch >= 256
    if name == "gemm_qmax_screen" or (name == "gemm_qmax_rowmax" and bf16 and Hl in (256, 512)):
        ku = Hl // 256
        return "screen_top2_kernel<%d, %d, %d, 0>(" % (ku, 2 // ku, 0 if name == "gemm_qmax_screen" else 1 if dbl else 2)
    if name == "gemm_qmax_rowmax":
        return "gemm_colmax_persistent_kernel<2, 2, %d, %d>(" % (1 if bf16 else 0, 1 if dbl else 0)
    if name == "gemm_hidden_fwd" and not bf16:
        # whole tiles: the persistent walk, gemm_fwd_persistent_kernel<TM, TN, 2> (64 x 128 tiles at width 256, 128 x 128 at 512)
        chains = 3 if dbl else 2
        if minibatch % 128 == 0 and all(h % 128 == 0 for h in layers[2:-1]) and all(h % 32 == 0 for h in layers[1:-2]):
            t128 = (minibatch // 128) * (layers[2] // 128) * chains
            return "gemm_fwd_persistent_kernel<%s, 2>(" % ("2, 2" if t128 >= 512 else "1, 2")
        big = ((minibatch + 127) // 128) * ((layers[2] + 127) // 128) * chains >= 512
        return "gemm_f32_kernel<0, 0, 1, %s, 0>(" % ("2, 2" if big else "1, 1")
    if name == "gemm_hidden_fwd@select" and not bf16:
        if k == 2:
            return "gemm_f32_kernel<0, 0, 4, 1, 1, 0>("       # one hidden product per ply, the select head riding on it
        return ["gemm_f32_kernel<0, 0, 1, 1, 1, 0>(", "gemm_f32_kernel<0, 0, 4, 1, 1, 0>("]
    if name == "qmax_refine":
        return "qmax_refine2_kernel<" if Hl in (256, 512) else "qmax_refine_kernel<"
    if name == "td_tail_l0":
        return "td_tail_kernel<%du, %s>(" % (TAIL_L0, "true" if mfma else "false")
    if name == "td_tail_deltas":
        if k < 2:
            return None
        plain = "td_tail_kernel<%du, false>(" % TAIL_DELTAS
        last = "td_tail_kernel<%du, false>(" % (TAIL_DELTAS_SEL if mfma else TAIL_DELTAS)    # the launch that makes delta_0 carries the selector words
        return last if k == 2 else ([plain, last] if mfma else plain)
    if name == "l0_grad_segsum" and mfma:
        return "l0_grad_mfma_kernel<0>("
    if name == "l0_delta_split":
        return "delta_split_kernel("
    if name == "l0_sel_words":
        return "l0_sel_kernel("
    return ROCPROF_NAMES.get(name)


def match_kernel(printed, want):
    """Does the kernel name rocprofv3 printed belong to the instance `want` (rocprof_kernel)?"""
    p = printed
    for pre in ("void ", "xq::"):
        if p.startswith(pre):
            p = p[len(pre):]
    return p.startswith(want)


def newest_profile_set(root, config=2):
    """(tag, kernel_stats.csv, pmc_hbm_traffic.json) of the newest COMPLETE profile set of a configuration under profiles/ — both files
    from the same rNN_x tag, i.e. the same build and bench command.  bench.py takes every `traffic` figure of a line from this one set
    (or none): no mixing across builds."""
    import glob, os, re
    suffix = "" if config == 2 else "_config%d" % config
    best = None
    for pmc in glob.glob(os.path.join(root, "profiles", "r*_pmc_hbm_traffic.json")):
        m = re.match(r"(r\d+_[a-z0-9]+)(_config\d+)?_pmc_hbm_traffic\.json$", os.path.basename(pmc))
        if not m or (m.group(2) or "") != suffix:
            continue
        stats = os.path.join(root, "profiles", m.group(1) + suffix + "_kernel_stats.csv")
        if os.path.exists(stats) and (best is None or m.group(1) > best[0]):
            best = (m.group(1), stats, pmc)
    return best


def pick_splits(M, N, K):
    """xq_dqn.hip::pick_splits + launch_gemm's rounding of the k-chunk to whole 32-deep k-tiles."""
    tiles = ((M + 63) // 64) * ((N + 63) // 64)
    s = (512 + tiles - 1) // tiles
    s = max(1, min(s, max(1, K // 128), 32))
    chunk = ((K + s - 1) // s + 31) // 32 * 32
    return (K + chunk - 1) // chunk


def step_work(layers, minibatch, n_games, plies=1, bf16=False, bf16_bwd=False, td="online", screened=True, derive=True,
              prioritized=False, l0_mfma=True, optimizer="sgd", grad_clip=False, soft_target=False, n_step=1,
              mirror=False, bootstrap="all", colour_swap=False, view=False):
    """{bracket name: dict(flops, hbm_bytes, bound, peak, peak_unit, what)} for one training step of the given configuration.
    optimizer="adam" (xq_dqn_set_optimizer): adam_apply stands in place of sgd_apply; the default step knows no adam_apply.
    grad_clip=True (xq_dqn_set_grad_clip): grad_norm stands in front of the apply and takes the slab sums over from it; the default
    step knows no grad_norm.
    soft_target=True (xq_dqn_set_target_tau in (0, 1), the target net in step with the online net outside the TD segments): the apply
    kernel also reads and writes the touched part of the target net (and writes its bf16 shadow); no bracket of its own.
    n_step > 1 (xq_replay_set_n_step): nstep_assemble stands in front of the step and, on a prioritized draw, per_writeback behind it;
    the default step knows neither.
    mirror=True (xq_replay_set_mirror with prob > 0): mirror_stage stands in front of the step (behind nstep_assemble when n_step > 1)
    and, on a prioritized draw with n_step == 1, per_writeback behind it; the default step knows no mirror_stage.
    bootstrap="legal" (xq_dqn_set_td_bootstrap, fp32 nets): gemm_legal_head and legal_qmax stand in place of the max pass over the 8100
    outputs (never screened), td_target_delta behind them, and legal_side_stage in front of a staged (n-step, mirror) batch; the default
    step knows none of them.
    colour_swap=True (xq_replay_set_colour_swap with prob > 0): colour_swap_stage stands in front of the step (behind nstep_assemble and
    mirror_stage when they are on) and, on a prioritized draw that nothing else stages, per_writeback behind it; under
    bootstrap="legal" it stages the side bytes too and legal_side_stage is not launched; the default step knows no colour_swap_stage.
    view=True (xq_trainer_set_view(XQ_VIEW_MOVER); not together with colour_swap): mover_view_stage stands in front of the step as the
    last staging transform and, on a prioritized draw that nothing else stages, per_writeback behind it; under bootstrap="legal" it
    stages the side bytes (0) and legal_side_stage is not launched; view_boards stands in front of the select chain; the default step
    knows neither."""
    if view and colour_swap:
        raise ValueError("view and colour_swap exclude each other (xq_dqn_td_grads_replay refuses the pair)")
    if bootstrap not in ("all", "legal"):
        raise ValueError("bootstrap: 'all' or 'legal'")
    legal = bootstrap == "legal"
    if legal and bf16:
        raise ValueError("bootstrap='legal' needs an fp32 net")
    screened = screened and not legal
    h = list(layers[1:-1])
    H1, Hl, k = h[0], h[-1], len(h)
    B, n = minibatch, n_games
    dbl = td == "double"
    chains = 3 if dbl else 2
    fa = 2 if bf16 else 4                               # bytes of an activation the forward kernels read
    mm_peak = PEAK_BF16_MFMA_TFLOPS if bf16 else PEAK_F32_MFMA_TFLOPS
    w = {}
    mfma0 = l0_mfma and H1 % 64 == 0 and B >= 256       # layer-0 gradient on the matrix pipe (xq_l0grad.hip.h; library default)

    def put(name, flops, by, bound, what, peak=None):
        if bound == "mfma":
            pk, unit = (peak or mm_peak), "TFLOP/s"
        else:
            pk, unit = PEAK_HBM_GBS, "GB/s"
        w[name] = dict(flops=float(flops), hbm_bytes=float(by), bound=bound, peak=pk, peak_unit=unit, what=what)

    # ---- TD step, handle's stream --------------------------------------------------------------------------------------------
    gathered = chains - (1 if derive and not dbl else (1 if derive and bf16 else 0))
    rows = 32 * gathered + (4 if derive else 0)         # ~32 occupied squares per gathered state, ~4 changed rows for a derived one
    put("l0_forward_gather", 2.0 * B * rows * H1,
        B * (chains * 48 + 48) + STATE * H1 * fa * (2 if dbl or td == "target" else 1) + chains * B * H1 * (4 if not bf16 else 2) +
        (B * H1 * 4 if bf16 else 0) + (96 * Hl * 6 if screened else 0),
        "hbm", "layer 0 of the forward chains as a gather of W0^T rows (L2-resident) + the minibatch's boards; "
               "s' derived from s when the TD rule allows")
    if k >= 2:
        fl = by = 0.0
        for l in range(1, k):
            fl += 2.0 * B * h[l - 1] * h[l] * chains
            by += chains * B * (h[l - 1] * fa + h[l] * (4 if not bf16 else 2)) + h[l - 1] * h[l] * fa * (2 if dbl or td == "target" else 1)
            if bf16:
                by += B * h[l] * 4                       # the s chain keeps an fp32 copy for the backward pass
        if screened:
            by += B * Hl * 2                             # bf16 fragment-order copy of a_last(s') for the screening pass
        put("gemm_hidden_fwd", fl / (k - 1), by / (k - 1), "mfma",
            "hidden products of the %d forward chains grouped in one launch per layer, bias + tanh epilogue" % chains)
    G = 2 * ((NO + 63) // 64)
    if legal:
        # the 96-row head of s' as k-slabs (q_head's split), once per net a Double-DQN step asks (online selects, target evaluates);
        # per row of legal_qmax: the board and 6 B of fields, the slabs of both heads, the 96 pre-activations and 12 B out
        nets = 2 if dbl else 1
        nslabs = min(Hl // 64, 8) if B >= 2048 and Hl % 128 == 0 else 1
        put("gemm_legal_head", 2.0 * B * 96 * Hl, B * Hl * 4 + 96 * Hl * 4 + nslabs * B * 96 * 4, "mfma",
            "pre-activations of outputs 0..95 for s' as k-slabs, per launch (%d per step)" % nets)
        put("legal_qmax", 0.0, B * (48 + 6 + 384.0 * nets * nslabs + 384 + 12), "hbm",
            "move generation for the side to move in s' and the greedy pick over z[to] of its moves: the legal-move bootstrap")
        put("td_target_delta", 4.0 * B * Hl, 2 * B * Hl * 4 + 32 * B, "hbm", "Q(s,a), y, output delta, top hidden delta")
    elif screened:
        put("gemm_qmax_screen", 2.0 * NO * B * Hl, NO * Hl * 2 + B * Hl * 2 + 2 * G * B * 4 + 16 * B * 4 + B * 4, "mfma",
            "exact screen of max_a' Q(s'): all 8100 outputs once on bf16 MFMA, top-2 per 32-output group", PEAK_BF16_MFMA_TFLOPS)
        td_in_refine = Hl == 256 and not prioritized and not bf16_bwd
        by = 16 * B * 4 + 2 * G * B * 4 / 16.0 + B * Hl * 4
        if td_in_refine:
            by += 2 * B * Hl * 4 + 24 * B                # a_last(s) in, top hidden delta out, action / reward / done / y / delta
        put("qmax_refine", 2.0 * B * Hl * (3 if td_in_refine else 1), by, "hbm",
            "fp32 re-evaluation of the screened candidates" + (" + TD target, output delta and top hidden delta" if td_in_refine else ""))
        if not td_in_refine:
            put("td_target_delta", 4.0 * B * Hl, 2 * B * Hl * 4 + 32 * B, "hbm", "Q(s,a), y, output delta, top hidden delta")
    else:
        fe = 2 if bf16 else 4
        tiles_m = (NO + 127) // 128
        put("gemm_qmax_rowmax", 2.0 * NO * B * Hl, fe * (NO * Hl + B * Hl) + 2 * tiles_m * B * 4 * (2 if dbl else 1), "mfma",
            "%s_a' Q(s') over all 8100 outputs, Q never written" % ("argmax" if dbl else "max"))
        put("colmax_reduce", B * 2.0 * tiles_m, 2 * tiles_m * B * 4 * (2 if dbl else 1) + 4 * B * 4 * 2, "hbm", "fold of the partial maxima")
        put("td_target_delta", 4.0 * B * Hl * (2 if dbl else 1), (2 + (1 if dbl else 0)) * B * Hl * 4 + 32 * B, "hbm",
            "Q(s,a), y, output delta, top hidden delta")
    # gradient half: fused launches (fp32 nets) — per launch means
    nch_out = (B + 255) // 256
    out_fl, out_by = 2.0 * B * Hl, B * Hl * 4 + 8 * B + nch_out * (96 * Hl + 96) * 4
    if not bf16:
        if k >= 2:
            fl = by = 0.0
            launches = k - 1
            for l in range(k - 2, -1, -1):               # delta_l from delta_{l+1}
                fl += 2.0 * B * h[l + 1] * h[l]
                by += B * h[l + 1] * 4 + h[l] * h[l + 1] * 4 + 2 * B * h[l] * 4
                if not (k == 2):                         # weight gradient of layer l+1 rides beside the delta product (3+ hidden layers)
                    sp = pick_splits(h[l + 1], h[l], B)
                    fl += 2.0 * h[l + 1] * h[l] * B
                    by += sp * h[l + 1] * h[l] * 4       # (its operands are the delta product's own)
            fl += out_fl; by += out_by
            put("td_tail_deltas", fl / launches, by / launches, "hbm",
                "fused launch: hidden delta product || weight-gradient product of the layer above || output-layer segmented sums")
        chunk = 2048 if B >= 16384 else 1024
        nch = (B + chunk - 1) // chunk
        kpad = nch * chunk
        if mfma0:
            # one-hot^T x delta_0: 80 tiles of 16 rows of gW0^T (1260 rows packed) x H1 columns x kpad samples x 3 bf16 planes of delta_0 (what the pipe executes;
            # the useful part is the ~32 occupied (square, piece) pairs per sample).  Bytes: the three planes and the selector words
            # in, delta_0 itself for the bias sums, the chunk partial sums out.
            fl = 2.0 * 80 * 16 * H1 * kpad * 3
            by = 6.0 * H1 * kpad + 4.0 * 96 * kpad + B * H1 * 4 + nch * STATE * H1 * 4
        else:
            fl = 2.0 * B * 32 * H1
            by = B * H1 * 4 + 48 * B + nch * STATE * H1 * 4
        if k == 2:                                       # the one weight-gradient product of a 2-hidden-layer net rides here
            sp = pick_splits(h[1], h[0], B)
            fl += 2.0 * h[1] * h[0] * B
            by += B * (h[0] + h[1]) * 4 + sp * h[0] * h[1] * 4
        if k == 1:
            fl += out_fl; by += out_by
        R = max(1, min(64, B // 64))
        by += R * sum(h) * 4
        fl += B * sum(h)
        put("td_tail_l0", fl, by, "hbm",
            "fused launch: layer-0 gradient " + ("as the exact product one-hot^T x delta_0 on the bf16 matrix pipe (3-term split) || "
                                                 if mfma0 else "as per-(square, piece) segmented sums of delta rows || ")
            + ("hidden weight-gradient product || " if k == 2 else "") + "bias column sums")
        if mfma0:
            w["td_tail_l0"]["mfma_bf16_flops"] = 2.0 * 80 * 16 * H1 * kpad * 3
            if "td_tail_deltas" in w:                    # the launch that makes delta_0 also writes its planes and the selector words
                w["td_tail_deltas"]["hbm_bytes"] += (6.0 * H1 * kpad + 4.0 * 96 * kpad + 48 * B) / max(1, k - 1)
        slabs = nch * STATE * H1 + nch_out * (96 * Hl + 96) + R * sum(h)
        for l in range(1, k):
            slabs += pick_splits(h[l], h[l - 1], B) * h[l] * h[l - 1]
        touched = STATE * H1 + sum(h[l] * h[l - 1] for l in range(1, k)) + 96 * Hl + 96 + sum(h)
        put("sgd_apply", 2.0 * touched, 4 * (slabs + 2 * touched), "hbm", "ordered sum of every partial-sum slab + SGD step on the touched parameters")
    else:
        # bf16 net (and xq_dqn_set_td_tail(0)): the same work as kernels of their own on two streams.  bf16 operands where the backward
        # products run on the bf16 loop (XQ_PRECISION_BF16_FULL), fp32 sums everywhere.
        eb = 2 if bf16_bwd else 4
        if k >= 2:
            fl = by = 0.0
            for l in range(k - 2, -1, -1):
                fl += 2.0 * B * h[l + 1] * h[l]
                by += B * h[l + 1] * eb + h[l] * h[l + 1] * eb + B * h[l] * (eb + 4 + (2 if bf16_bwd else 0))
            put("gemm_hidden_delta", fl / (k - 1), by / (k - 1), "mfma", "hidden delta product (delta_{l+1} . weight view) (1 - a^2)",
                PEAK_BF16_MFMA_TFLOPS if bf16_bwd else PEAK_F32_MFMA_TFLOPS)
            fl = by = 0.0
            for l in range(1, k):
                sp = max(1, min(16, 256 // max(1, (h[l] // 256) * (h[l - 1] // 128)))) if bf16_bwd else pick_splits(h[l], h[l - 1], B)
                fl += 2.0 * h[l] * h[l - 1] * B
                by += B * (h[l] + h[l - 1]) * eb + sp * h[l] * h[l - 1] * 4
            put("gemm_grad_hidden", fl / (k - 1), by / (k - 1), "mfma", "hidden weight-gradient product, split-K slabs",
                PEAK_BF16_MFMA_TFLOPS if bf16_bwd else PEAK_F32_MFMA_TFLOPS)
        chunk = 2048 if B >= 16384 else 1024
        nch = (B + chunk - 1) // chunk
        if mfma0:
            kpad = nch * chunk
            put("l0_grad_segsum", 2.0 * 80 * 16 * H1 * kpad * 3, 6.0 * H1 * kpad + 4.0 * 96 * kpad + nch * STATE * H1 * 4, "mfma",
                "layer-0 gradient as the exact product one-hot^T x delta_0 on the bf16 matrix pipe (3-term split)", PEAK_BF16_MFMA_TFLOPS)
            put("l0_delta_split", 8.0 * B * H1, B * H1 * 4 + 6.0 * H1 * kpad, "hbm", "delta_0 -> three transposed bf16 planes (hi, mid, lo)")
            put("l0_sel_words", 0.0, 48 * B + 4.0 * 96 * kpad, "hbm", "boards -> selector half-words of the one-hot operand")
        else:
            put("l0_grad_segsum", 2.0 * B * 32 * H1, B * H1 * 4 + 48 * B + nch * STATE * H1 * 4, "hbm",
                "layer-0 gradient as per-(square, piece) segmented sums of delta rows (L2 gather)")
        put("out_grad_segsum", out_fl, out_by, "hbm", "output-layer gradient rows 0..95 as segmented sums by action")
        R = max(1, min(64, B // 64))
        put("bias_grad_colsum", float(B * sum(h)), B * sum(h) * 4 + R * sum(h) * 4, "hbm", "bias gradients: column sums of every hidden delta")
        slabs = nch * STATE * H1 + nch_out * (96 * Hl + 96) + R * sum(h)
        for l in range(1, k):
            sp = max(1, min(16, 256 // max(1, (h[l] // 256) * (h[l - 1] // 128)))) if bf16_bwd else pick_splits(h[l], h[l - 1], B)
            slabs += sp * h[l] * h[l - 1]
        touched = STATE * H1 + sum(h[l] * h[l - 1] for l in range(1, k)) + 96 * Hl + 96 + sum(h)
        put("sgd_apply", 2.0 * touched, 4 * (slabs + 2 * touched) + (2 * touched if bf16 else 0), "hbm",
            "ordered sum of every partial-sum slab + SGD step on the touched parameters (+ their bf16 shadow)")
    if optimizer == "adam":
        # the SGD kernel's bytes + m and v read and written: 16 B per touched element; ~12 fp32 operations per element
        sgd = w.pop("sgd_apply")
        put("adam_apply", 12.0 * touched, sgd["hbm_bytes"] + 16 * touched, "hbm",
            "ordered sum of every partial-sum slab + Adam step on the touched parameters and their two moments" + (" (+ their bf16 shadow)" if bf16 else ""))
    elif optimizer != "sgd":
        raise ValueError("optimizer: 'sgd' or 'adam'")
    if grad_clip:
        # every slab read once and the gradient buffer written (the squares are summed on the way, in fp64); the apply kernel behind
        # it reads the buffer instead of the slabs
        put("grad_norm", 3.0 * touched + slabs, 4 * (slabs + touched), "hbm",
            "ordered sum of every partial-sum slab into the gradient buffer + fp64 sum of its squares (global-norm clipping)")
        w["adam_apply" if optimizer == "adam" else "sgd_apply"]["hbm_bytes"] -= 4 * (slabs - touched)
    if soft_target:
        # theta- += tau (theta - theta-) on the values the apply holds in registers: one read and one write of the touched target
        a = w["adam_apply" if optimizer == "adam" else "sgd_apply"]
        a["flops"] += 2.0 * touched
        a["hbm_bytes"] += 8 * touched + (2 * touched if bf16 else 0)
        a["what"] += " + soft update of the touched target parameters"
    if n_step > 1:
        # per row: action, reward and done of the n chain elements and two boards in, two boards and 21 B of row fields out
        put("nstep_assemble", 2.0 * B * (n_step - 1), B * (9.0 * n_step + 4 * 48 + 21), "hbm",
            "gather of the minibatch's n-step transitions into the staging batch the TD step reads")
        if prioritized:
            put("per_writeback", 0.0, 20.0 * B, "hbm", "TD-error priorities of a prioritized n-step draw back to the sampled slots")
    if mirror:
        # per row, from the ring: two boards and 9 B in, two boards, 9 B, the slot and the flag out; in place behind nstep_assemble: two
        # boards and the action in, two boards, the action and the flag out
        put("mirror_stage", 0.0, B * (215.0 if n_step == 1 else 201.0), "hbm",
            "left-right reflection of the flagged minibatch rows in the staging batch the TD step reads")
        if prioritized and n_step == 1:
            put("per_writeback", 0.0, 20.0 * B, "hbm", "TD-error priorities of a prioritized mirrored draw back to the sampled slots")
    if colour_swap:
        # per row: the mirror's bytes — from the ring when it is the first staging transform, in place behind nstep_assemble or
        # mirror_stage; under the legal bootstrap also the side byte: the ring's byte in and the staged one out, in place the 4 B of the
        # slot it is read at as well (legal_side_stage is then not launched)
        first = n_step == 1 and not mirror
        put("colour_swap_stage", 0.0, B * ((215.0 if first else 201.0) + ((2.0 if first else 6.0) if legal else 0.0)), "hbm",
            "exchange of the colours (row -> 9 - row, Red <-> Black) of the flagged minibatch rows in the staging batch the TD step reads")
        if prioritized and first:
            put("per_writeback", 0.0, 20.0 * B, "hbm", "TD-error priorities of a prioritized colour-swapped draw back to the sampled slots")
    if view:
        # per row: the mirror's bytes with a second flag out, the ring's two side bytes in, in place the 8 B of the two slots they are read
        # at; under the legal bootstrap the staged side byte out (legal_side_stage is then not launched)
        first = n_step == 1 and not mirror
        put("mover_view_stage", 0.0, B * ((218.0 if first else 212.0) + (1.0 if legal else 0.0)), "hbm",
            "mover view of the minibatch in the staging batch the TD step reads: s and the action by who moved, s' by who moves next")
        if prioritized and first:
            put("per_writeback", 0.0, 20.0 * B, "hbm", "TD-error priorities of a prioritized view-mode draw back to the sampled slots")
    if legal and (n_step > 1 or mirror) and not colour_swap and not view:
        # per staged row: the slot whose side it takes (4 B), the ring's byte, the staged byte
        put("legal_side_stage", 0.0, 6.0 * B, "hbm", "side to move in s' of every staged row, from the ring's column (legal-move bootstrap)")
    nw =STATE * H1 + sum(h[l] * h[l - 1] for l in range(1, k)) + Hl * NO
    nb = sum(h) + NO
    put("target_sync_copy", 0.0, 8.0 * (nw + nb), "hbm", "updateTargetNetwork(): device copy of all parameters")
    # ---- select chain (collect stream): one ply in every game ---------------------------------------------------------------------
    put("l0_forward_gather@select", 2.0 * n * 32 * H1, 48 * n + STATE * H1 * fa + n * H1 * (2 if bf16 else 4), "hbm",
        "layer 0 of Q(s) for the boards of every game (gather)")
    ride = (not bf16) and k >= 2 and n >= 2048 and n % 64 == 0 and Hl % 128 == 0
    if k >= 2:
        fl = by = 0.0
        for l in range(1, k):
            fl += 2.0 * n * h[l - 1] * h[l]
            by += n * h[l - 1] * fa + h[l - 1] * h[l] * fa
            if l == k - 1 and ride:
                fl += 2.0 * n * Hl * 128
                by += (Hl // 64) * n * 96 * 4 + 128 * Hl * 4
            else:
                by += n * h[l] * (2 if bf16 else 4)
        put("gemm_hidden_fwd@select", fl / (k - 1), by / (k - 1), "mfma",
            "hidden products of the select chain" + ("; the last one carries the select head (Q[0..95] as k-slabs)" if ride else ""))
    if not ride:
        put("gemm_q90_select@select", 2.0 * n * Hl * 96, n * Hl * fa + 96 * Hl * fa + n * 96 * 4, "mfma", "select head Q(s)[0..95]")
    if view:
        put("view_boards@select", 0.0, (48.0 + 16.0 + 48.0) * n, "hbm", "view(board, side to move) of every game's board for the select chain")
    put("env_selfplay_step", 0.0, float(ENV_BYTES_PER_GAME) * n, "hbm",
        "fused self-play ply: legal moves, epsilon-greedy select, movePiece, reward, game over, auto-reset, transition -> ring")
    return w


def price(entry, avg_us):
    """achieved / frac of one kernel at its measured mean launch duration."""
    t = avg_us * 1e-6
    if entry["bound"] == "mfma":
        ach = entry["flops"] / t / 1e12
    else:
        ach = entry["hbm_bytes"] / t / 1e9
    return ach, ach / entry["peak"]
