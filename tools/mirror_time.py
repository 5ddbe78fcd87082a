"""What mirror augmentation costs when it is on, on one GPU at the headline configuration (8192 games, 1260-256-256-8100, ring of 1 M,
minibatch 8192, overlapped trainer, exact screening, layer 0 of s' derived, through the Python Trainer).

    python tools/mirror_time.py [--steps 200] [--warmup 100] [--reps 4] [--prob 0.5] [--ring 1048576]

One process, one trainer; Trainer.set_mirror alternates 0, prob, 0, prob, .. --reps times each.  Per leg one JSON line: wall ms/step of
--steps steps and, from the kernel statistics of a further --steps steps, the exact-event time per launch of mirror_stage and of every
other bracketed kernel of the step (the step reads a staged, contiguous batch in place of the implicit draw's ring slots, so its gather
moves too) and their sum.  profiles/NOTES.md ("Mirror augmentation") says what to set it against."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NET = (1260, 256, 256, 8100)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--prob", type=float, default=0.5)
    ap.add_argument("--ring", type=int, default=1 << 20)
    args = ap.parse_args()
    import cn_chess_ai_amd as xq
    from cn_chess_ai_amd import _capi
    n, cap = 8192, args.ring
    cfg = xq.TrainerConfig(n_games=n, layer_sizes=NET, learning_rate=0.001, gamma=0.99, epsilon=0.1, replay_capacity=cap, minibatch=n,
                           td_net=_capi.TD_ONLINE_NET, backprop_mode=_capi.BACKPROP_REFERENCE, target_sync_interval=10, mean_gradient=1,
                           seed=0x5EED, first_game_id=0, overlap_collect=1, collects_per_update=1)
    t = xq.Trainer(cfg)
    t.dqn.set_qmax_mode(_capi.QMAX_SCREENED)
    t.dqn.set_l0_derive(True)
    t.dqn.set_fused_apply(True)
    t.random_plies(300)
    for _ in range(cap // n):
        t.collect()
    t.step(args.warmup)
    t.synchronize()
    for rep in range(args.reps):
        for prob in (0.0, args.prob):
            t.set_mirror(prob)
            t.step(10)
            t.synchronize()
            t0 = time.perf_counter()
            t.step(args.steps)
            t.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            t.dqn.kernel_stats(2)
            t.step(args.steps)
            st = {s["name"]: s for s in t.dqn.kernel_stats(0)}
            out = dict(rep=rep, mirror=prob, ms_per_step=round(ms, 4), calls=t.replay.mirror[1],
                       step_kernel_sum_us=round(1e3 * sum(s["ms"] for s in st.values()) / args.steps, 2),
                       kernels_us={k: round(1e3 * s["ms"] / s["launches"], 2) for k, s in st.items()})
            if "mirror_stage" in st:
                out["mirror_stage_us"] = round(st["mirror_stage"]["ms"] * 1e3 / st["mirror_stage"]["launches"], 3)
                out["mirror_stage_launches"], out["mirror_stage_exact"] = st["mirror_stage"]["launches"], st["mirror_stage"]["exact"]
                out["flagged"] = int(t.dqn.last_mirror(n)["flags"].sum())
            print(json.dumps(out), flush=True)
    t.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
