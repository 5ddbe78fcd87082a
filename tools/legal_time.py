"""What the TD step costs under the legal-move bootstrap, beside the default (screened, all-outputs) step, on one GPU at the headline shapes
(minibatch 8192, 1260-256-256-8100, exact screening, layer 0 of s' derived, fused apply).

    python tools/legal_time.py [--steps 200] [--warmup 50] [--reps 4] [--td-net 0]
    python tools/legal_time.py --trainer [--steps 200] [--warmup 100] [--reps 3] [--ring 1048576]
    python tools/legal_time.py --zero-sum [--steps 200] [--warmup 50] [--reps 4] [--td-net 0]

One process, one handle, one batch of 8192 real self-play transitions held in HBM (boards after 40 random plies, the side to move in s'
from the env's own record); DQN.set_td_bootstrap alternates "all", "legal", .. --reps times each.  The step is xq_dqn_td_grads(_sided) +
xq_dqn_apply_grads on that batch with nothing beside it (no collect, no select chain).  Per leg one JSON line: wall ms/step of --steps
steps and, from the kernel statistics of a further --steps steps, the time per launch of every bracketed kernel (legal_qmax and
gemm_legal_head among them) and their sum.
--zero-sum: the two legs are the legal step without and with the zero-sum target (DQN.set_zero_sum; the kernel then writes -inf in place of
0 for a side without a move and the step's discount is negative: no launch changes).
--trainer: the whole training step instead, through two Trainers of the headline configuration in one process (8192 games, ring of 1 M,
overlapped collect) — one under "all", one under "legal" (the setting must precede a trainer's first collect) — timed alternately.
profiles/NOTES.md ("Legal-move bootstrap") says what to set it against."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NET = (1260, 256, 256, 8100)


def pack(boards):
    """[n][90] piece codes -> [n][12] uint32, square s in nibble s & 7 of word s >> 3"""
    b = np.zeros((len(boards), 96), np.uint32)
    b[:, :90] = boards
    return (b.reshape(-1, 12, 8) << (4 * np.arange(8, dtype=np.uint32))).sum(axis=2).astype(np.uint32)


def trainer_legs(args):
    import cn_chess_ai_amd as xq
    from cn_chess_ai_amd import _capi
    n, cap = 8192, args.ring
    ts = {}
    for kind in ("all", "legal"):
        cfg = xq.TrainerConfig(n_games=n, layer_sizes=NET, learning_rate=0.001, gamma=0.99, epsilon=0.1, replay_capacity=cap, minibatch=n,
                               td_net=_capi.TD_ONLINE_NET, backprop_mode=_capi.BACKPROP_REFERENCE, target_sync_interval=10,
                               mean_gradient=1, seed=0x5EED, first_game_id=0, overlap_collect=1, collects_per_update=1)
        t = xq.Trainer(cfg)
        t.dqn.set_qmax_mode(_capi.QMAX_SCREENED)
        t.dqn.set_l0_derive(True)
        t.dqn.set_fused_apply(True)
        t.set_td_bootstrap(kind)
        t.random_plies(300)
        for _ in range(cap // n):
            t.collect()
        t.step(args.warmup)
        t.synchronize()
        ts[kind] = t
    for rep in range(args.reps):
        for kind, t in ts.items():
            t.step(10)
            t.synchronize()
            t0 = time.perf_counter()
            t.step(args.steps)
            t.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            t.dqn.kernel_stats(2)
            t.step(args.steps)
            st = {s["name"]: s for s in t.dqn.kernel_stats(0)}
            print(json.dumps(dict(rep=rep, trainer=kind, ms_per_step=round(ms, 4),
                                  kernels_us={k: round(1e3 * s["ms"] / s["launches"], 2) for k, s in st.items()})), flush=True)
    for t in ts.values():
        t.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--td-net", type=int, default=0)
    ap.add_argument("--trainer", action="store_true")
    ap.add_argument("--zero-sum", action="store_true")
    ap.add_argument("--ring", type=int, default=1 << 20)
    args = ap.parse_args()
    if args.trainer:
        return trainer_legs(args)
    import torch
    import cn_chess_ai_amd as xq
    from cn_chess_ai_amd import _capi
    n = 8192
    env = xq.VecEnv(n, seed=0x5EED)
    for _ in range(40):
        env.selfplay_step(None)
    S, meta = env.get_state()
    res = env.selfplay_step(None)
    S2, _ = env.get_state()
    env.close()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t_s, t_s2 = dev(pack(S).view(np.int32)), dev(pack(S2).view(np.int32))
    t_a = dev(np.where(res["action"] >= 0, res["action"] % 90, -1).astype(np.int32))
    t_r = dev((res["reward"] / 100.0).astype(np.float32))
    t_d = dev(res["done"].astype(np.uint8))
    t_p = dev((1 - meta[:, 1]).astype(np.uint8))
    torch.cuda.synchronize()
    d = xq.DQN(NET, 0.001, 0.99, seed=1)
    d.set_qmax_mode(_capi.QMAX_SCREENED)
    d.set_l0_derive(True)
    d.set_fused_apply(True)
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def steps(k, legal):
        for _ in range(k):
            if legal:
                _capi.call("xq_dqn_td_grads_sided", d.handle, ptr(t_s), ptr(t_s2), ptr(t_a), ptr(t_r), ptr(t_d), ptr(t_p), None, n,
                           args.td_net, _capi.BACKPROP_REFERENCE)
            else:
                _capi.call("xq_dqn_td_grads", d.handle, ptr(t_s), ptr(t_s2), ptr(t_a), ptr(t_r), ptr(t_d), None, n, args.td_net,
                           _capi.BACKPROP_REFERENCE)
            d.apply_grads(0.001, 1.0 / n)
        _capi.call("xq_stream_synchronize", C.c_void_p(d.stream()))

    steps(args.warmup, False)
    for rep in range(args.reps):
        for kind, zero_sum in ((("legal", False), ("legal", True)) if args.zero_sum else (("all", False), ("legal", False))):
            d.set_td_bootstrap(kind)
            d.set_zero_sum(zero_sum)
            legal = kind == "legal"
            steps(10, legal)
            t0 = time.perf_counter()
            steps(args.steps, legal)
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            d.kernel_stats(2)
            steps(args.steps, legal)
            st = {s["name"]: s for s in d.kernel_stats(0)}
            out = dict(rep=rep, bootstrap=kind, zero_sum=zero_sum, td_net=args.td_net, ms_per_step=round(ms, 4),
                       step_kernel_sum_us=round(1e3 * sum(s["ms"] for s in st.values()) / args.steps, 2),
                       kernels_us={k: round(1e3 * s["ms"] / s["launches"], 2) for k, s in st.items()})
            if legal:
                L = d.last_legal(n, z96=False)
                out["rows_without_a_move"] = int((L["n_moves"] == 0).sum())
                out["rows_with_moves"], out["mean_moves"] = int((L["n_moves"] > 0).sum()), round(float(L["n_moves"][L["n_moves"] > 0].mean()), 1)
            print(json.dumps(out), flush=True)
    d.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
