"""colour_swap_stage_kernel alone, both forms, beside mirror_stage_kernel on the same box, ring and batch (8192 rows of a 64 K ring of
random boards, 1260-256-256-8100, uniform draw).

    python tools/colour_swap_time.py [--steps 60] [--warmup 10] [--reps 3] [--batch 8192] [--ring 65536]

One process, one ring, one Q-net.  Per leg one JSON line with the exact-event time per launch (kernel statistics) of the staging
kernels the leg launches:
    mirror         mirror_stage, gather form
    swap           colour_swap_stage, gather form
    both           mirror_stage gather, colour_swap_stage in place behind it
    nstep_mirror   mirror_stage in place behind nstep_assemble (n = 3)
    nstep_swap     colour_swap_stage in place behind nstep_assemble (n = 3)
    legal_swap     colour_swap_stage, gather form, staging the side byte too (legal-move bootstrap; ring tracks the side)
profiles/NOTES.md ("Colour-swap augmentation") says what to set it against."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NET = (1260, 256, 256, 8100)
LEGS = (("mirror", 1, 0.5, 0.0, False), ("swap", 1, 0.0, 0.5, False), ("both", 1, 0.5, 0.5, False), ("nstep_mirror", 3, 0.5, 0.0, False),
        ("nstep_swap", 3, 0.0, 0.5, False), ("legal_swap", 1, 0.0, 0.5, True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--ring", type=int, default=1 << 16)
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
    side = rng.integers(0, 2, cap).astype(np.uint8)
    rp = xq.ReplayBuffer(cap, seed=7)
    rp.track_next_player()
    rp.push(S, A, R, D, S2, next_player=side)
    d = xq.DQN(list(NET), 0.001, 0.99, seed=1)
    for rep in range(args.reps):
        for name, n, mirror, swap, legal in LEGS:
            rp.set_n_step(n, 1)
            rp.set_mirror(mirror)
            rp.set_colour_swap(swap)
            d.set_td_bootstrap("legal" if legal else "all")
            for k in range(args.warmup + args.steps):
                if k == args.warmup:
                    d.kernel_stats(2)
                rp.sample(B, host=False)
                d.td_grads_replay(rp, B)
                d.apply_grads(0.0, 1.0)
            st = {s["name"]: s for s in d.kernel_stats(0)}
            out = dict(rep=rep, leg=name, batch=B, ring=cap)
            for k in ("mirror_stage", "colour_swap_stage", "nstep_assemble", "legal_side_stage"):
                if k in st:
                    out[k + "_us"] = round(1e3 * st[k]["ms"] / st[k]["launches"], 3)
                    out[k + "_launches"], out[k + "_exact"] = st[k]["launches"], st[k]["exact"]
            print(json.dumps(out), flush=True)
    d.close()
    rp.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
