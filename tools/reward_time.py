"""What the delta reward rule costs in the collect's env launches, on one GPU at 8192 games (1260-256-256-8100, sequential trainer,
through the Python Trainer), in self-play and against uniform-random play.

    python tools/reward_time.py [--games 8192] [--collects 200] [--warmup 20] [--reps 4]

One process, one trainer per mode; Trainer.set_reward alternates "evaluate", "delta", .. --reps times each.  Per leg one JSON line: wall
ms per collect of --collects collects (select chain + env launches, the stream synchronised before and after) and, in self-play, from
the kernel statistics of a further --collects collects the exact-event time per launch of env_selfplay_step.  A versus collect is three
env launches (pre-move, learner, reply) which the handle does not bracket: there the wall time is the figure.  Expected: no difference
in self-play (one wave-uniform select in front of lane 0's store), and one 4-byte scalar load per game at the top of the reply launch of
versus, beside the board and meta loads.  profiles/NOTES.md ("Reward rule") says what was measured."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NET = (1260, 256, 256, 8100)
RULES = (("evaluate",), ("delta", 1e-3, 0.0, 1.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=8192)
    ap.add_argument("--collects", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=4)
    args = ap.parse_args()
    import cn_chess_ai_amd as xq
    from cn_chess_ai_amd import _capi
    n = args.games
    for mode, opp in (("selfplay", None), ("versus_random", "random")):
        cfg = xq.TrainerConfig(n_games=n, layer_sizes=NET, learning_rate=0.001, gamma=0.99, epsilon=0.1, replay_capacity=16 * n,
                               minibatch=n, td_net=_capi.TD_ONLINE_NET, backprop_mode=_capi.BACKPROP_REFERENCE, target_sync_interval=10,
                               mean_gradient=1, seed=0x5EED, first_game_id=0, overlap_collect=0, collects_per_update=1)
        t = xq.Trainer(cfg)
        t.random_plies(60)
        t.set_opponent(opp)
        for _ in range(args.warmup):
            t.collect()
        t.synchronize()
        for rep in range(args.reps):
            for rule in RULES:
                t.set_reward(*rule)
                for _ in range(5):
                    t.collect()
                t.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.collects):
                    t.collect()
                t.synchronize()
                ms = (time.perf_counter() - t0) * 1e3 / args.collects
                out = dict(mode=mode, rep=rep, reward=rule[0], games=n, collects=args.collects, ms_per_collect=round(ms, 4))
                if opp is None:
                    t.dqn.kernel_stats(2)
                    for _ in range(args.collects):
                        t.collect()
                    st = {s["name"]: s for s in t.dqn.kernel_stats(0)}
                    e = st.get("env_selfplay_step")
                    if e:
                        out["env_selfplay_step_us"] = round(1e3 * e["ms"] / e["launches"], 3)
                        out["env_launches"], out["env_exact"] = e["launches"], e["exact"]
                print(json.dumps(out), flush=True)
        t.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
