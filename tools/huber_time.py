"""The Huber TD loss on one GPU at the headline configuration (8192 games, 1260-256-256-8100, minibatch 8192, overlapped trainer, exact
screening, layer 0 of s' derived, through the Python Trainer).

    python tools/huber_time.py [--steps 200] [--warmup 100] [--reps 5] [--kappa 1.0]

One process, one trainer; the loss alternates squared, huber, squared, huber, .. --reps times each.  Per leg one JSON line: wall ms/step
of --steps steps and, from the kernel statistics of a further --steps steps, the exact-event time per launch of qmax_refine (which
carries the TD delta at this configuration) and of td_target_delta where it is launched; under Huber also the TD-error summary.
--td-tail 0 takes the delta out of the refine blocks, so that td_delta_kernel and its Huber twin are the ones timed."""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kappa", type=float, default=1.0)
    ap.add_argument("--td-tail", type=int, default=1)
    args = ap.parse_args()
    import cn_chess_ai_amd as xq
    from cn_chess_ai_amd import _capi
    n, cap = 8192, 1 << 18
    cfg = xq.TrainerConfig(n_games=n, layer_sizes=NET, learning_rate=0.001, gamma=0.99, epsilon=0.1, replay_capacity=cap, minibatch=n,
                           td_net=_capi.TD_ONLINE_NET, backprop_mode=_capi.BACKPROP_REFERENCE, target_sync_interval=10, mean_gradient=1,
                           seed=0x5EED, first_game_id=0, overlap_collect=1, collects_per_update=1)
    t = xq.Trainer(cfg)
    t.dqn.set_qmax_mode(_capi.QMAX_SCREENED)
    t.dqn.set_l0_derive(True)
    t.dqn.set_td_tail(bool(args.td_tail))
    t.random_plies(300)
    for _ in range(cap // n):
        t.collect()
    t.step(args.warmup)
    t.synchronize()
    for rep in range(args.reps):
        for loss in ("squared", "huber"):
            t.dqn.set_td_loss(loss, args.kappa)
            t.step(10)
            t.synchronize()
            t0 = time.perf_counter()
            t.step(args.steps)
            t.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            t.dqn.kernel_stats(2)
            t.step(args.steps)
            st = {s["name"]: s for s in t.dqn.kernel_stats(0)}
            out = dict(rep=rep, loss=loss, kappa=args.kappa, td_tail=args.td_tail, ms_per_step=round(ms, 4))
            for k in ("qmax_refine", "td_target_delta"):
                if k in st:
                    out[k + "_us"] = round(st[k]["ms"] * 1e3 / st[k]["launches"], 3)
                    out[k + "_launches"] = st[k]["launches"]
            if loss == "huber":
                out["stats"] = t.dqn.td_error_stats()
            print(json.dumps(out), flush=True)
    t.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
