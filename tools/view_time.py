"""view_boards_kernel and mover_view_stage_kernel alone, beside colour_swap_stage_kernel on the same box, ring and batch (8192 rows of a
64 K ring of random boards, 1260-256-256-8100, uniform draw), and the trainer's step with and without the mover view.

    python tools/view_time.py [--steps 60] [--warmup 10] [--reps 3] [--batch 8192] [--ring 65536] [--trainer-steps 300]

One process, one ring, one Q-net.  Per leg one JSON line with the exact-event time per launch (kernel statistics) of the staging
kernels the leg launches:
    swap           colour_swap_stage, gather form (the absolute view)
    view           mover_view_stage, gather form
    mirror_view    mover_view_stage in place behind mirror_stage
    nstep_view     mover_view_stage in place behind nstep_assemble (n = 3)
    legal_view     mover_view_stage, gather form, staging the side byte too (legal-move bootstrap)
then view_boards_kernel on --batch boards between two events of its own, and the wall time per iteration of two trainers in the headline
configuration (8192 games, minibatch 8192, ring of 64 collects, overlapped collect), absolute and mover, alternating.
profiles/NOTES.md ("Mover view") says what to set it against."""
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
LEGS = (("swap", 1, 0.0, 0.5, False, False), ("view", 1, 0.0, 0.0, True, False), ("mirror_view", 1, 0.5, 0.0, True, False),
        ("nstep_view", 3, 0.0, 0.0, True, False), ("legal_view", 1, 0.0, 0.0, True, True))


def time_view_boards(xq, B, steps, warmup, rng):
    import torch
    from cn_chess_ai_amd import _capi
    src = torch.from_numpy(rng.integers(0, 2 ** 31, (B, 12)).astype(np.int32) & 0x66666666).cuda()      # codes 0..6 in every nibble
    side = torch.from_numpy(rng.integers(0, 2, B).astype(np.uint8)).cuda()
    out = torch.empty_like(src)
    stream = torch.cuda.current_stream().cuda_stream
    us = []
    for k in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _capi.call("xq_view_boards_dev", C.c_void_p(src.data_ptr()), C.c_void_p(side.data_ptr()), B, C.c_void_p(out.data_ptr()),
                   C.c_void_p(stream))
        b.record()
        b.synchronize()
        if k >= warmup:
            us.append(1e3 * a.elapsed_time(b))
    return dict(leg="view_boards", boards=B, median_us=round(float(np.median(us)), 3), min_us=round(float(np.min(us)), 3),
                note="two event records around one launch: an upper bound")


def trainer_ms(xq, view, steps, warmup):
    from cn_chess_ai_amd import _capi
    n = 8192
    cfg = xq.TrainerConfig(n_games=n, layer_sizes=NET, learning_rate=1e-3, gamma=0.99, epsilon=0.1, replay_capacity=64 * n, minibatch=n,
                           td_net=_capi.TD_ONLINE_NET, backprop_mode=_capi.BACKPROP_REFERENCE, target_sync_interval=100, mean_gradient=1,
                           seed=0x5EED, first_game_id=0, overlap_collect=1, collects_per_update=1)
    t = xq.Trainer(cfg)
    t.dqn.set_qmax_mode(_capi.QMAX_SCREENED)
    if view:
        t.set_view("mover")
    t.step(warmup)
    t.synchronize()
    t0 = time.perf_counter()
    t.step(steps)
    t.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    t.close()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--ring", type=int, default=1 << 16)
    ap.add_argument("--trainer-steps", type=int, default=300)
    args = ap.parse_args()
    import cn_chess_ai_amd as xq
    rng = np.random.default_rng(3)
    cap, B = args.ring, args.batch
    S = np.zeros((cap, 90), np.uint8)
    S2 = np.zeros((cap, 90), np.uint8)
    for brd in (S, S2):                                                 # 16 pieces a side on random squares: the density of a real board
        for i in range(cap):
            brd[i, rng.choice(90, 32, replace=False)] = np.concatenate([rng.integers(1, 8, 16), rng.integers(8, 15, 16)])
    A = rng.integers(0, 90, cap).astype(np.int32)
    R = rng.uniform(-1, 1, cap).astype(np.float32)
    D = (rng.random(cap) < 0.02).astype(np.uint8)
    mover = rng.integers(0, 2, cap).astype(np.uint8)
    rp = xq.ReplayBuffer(cap, seed=7)
    rp.track_mover()
    rp.track_next_player()
    rp.push(S, A, R, D, S2, mover=mover, next_player=1 - mover)
    d = xq.DQN(list(NET), 0.001, 0.99, seed=1)
    for rep in range(args.reps):
        for name, n, mirror, swap, view, legal in LEGS:
            rp.set_n_step(n, 1)
            rp.set_mirror(mirror)
            rp.set_colour_swap(swap)
            d.set_view("mover" if view else "absolute")
            d.set_td_bootstrap("legal" if legal else "all")
            for k in range(args.warmup + args.steps):
                if k == args.warmup:
                    d.kernel_stats(2)
                rp.sample(B, host=False)
                d.td_grads_replay(rp, B)
                d.apply_grads(0.0, 1.0)
            st = {s["name"]: s for s in d.kernel_stats(0)}
            out = dict(rep=rep, leg=name, batch=B, ring=cap)
            for k in ("mirror_stage", "colour_swap_stage", "mover_view_stage", "nstep_assemble", "legal_side_stage"):
                if k in st:
                    out[k + "_us"] = round(1e3 * st[k]["ms"] / st[k]["launches"], 3)
                    out[k + "_launches"], out[k + "_exact"] = st[k]["launches"], st[k]["exact"]
            print(json.dumps(out), flush=True)
    d.close()
    rp.close()
    print(json.dumps(time_view_boards(xq, B, args.steps, args.warmup, rng)), flush=True)
    for rep in range(args.reps):
        for view in (False, True):
            print(json.dumps(dict(rep=rep, leg="trainer", view="mover" if view else "absolute", steps=args.trainer_steps,
                                  ms_per_step=round(trainer_ms(xq, view, args.trainer_steps, 20), 4))), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
