"""Does the colour swap change what the learner learns?  tools/learn_curve.py's recipe (versus training against uniform-random play,
delta(1e-3, 0, 1) reward, legal-move bootstrap, Adam, Huber, soft target, clip), trained once with Trainer.set_colour_swap(0) and once
with --prob (0.5), from the same seed, scored in the arena as training goes on.

    python tools/colour_swap_curve.py [--games 4096] [--iters 4000] [--every 500] [--pairs 2048] [--prob 0.5] [--out profiles/colour_swap_curve.json]

One seed, one opponent: a recorded result, not a gate.  profiles/NOTES.md ("Colour-swap augmentation") says what came out."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from learn_curve import NET, score  # noqa: E402

RULE = ("delta", 1e-3, 0.0, 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=4000)
    ap.add_argument("--every", type=int, default=500)
    ap.add_argument("--pairs", type=int, default=2048)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--prob", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colour_swap_curve.json"))
    args = ap.parse_args()
    import cn_chess_ai_amd as xq
    from cn_chess_ai_amd import _capi
    n = args.games
    recipe = dict(games=n, net=list(NET), ring=64 * n, minibatch=n, epsilon=0.1, optimizer="adam", lr=args.lr, loss="huber(1)",
                  bootstrap="legal", td_net="target", target_tau=0.01, grad_clip=10.0, gamma=0.99, opponent="random", seed=0x5EED,
                  reward=list(RULE), arena_pairs=args.pairs, arena_opening_plies=8, arena="greedy net against uniform-random play")
    legs = []
    for prob in (0.0, args.prob):
        cfg = xq.TrainerConfig(n_games=n, layer_sizes=NET, learning_rate=args.lr, gamma=0.99, epsilon=0.1, replay_capacity=64 * n,
                               minibatch=n, td_net=_capi.TD_TARGET_NET, backprop_mode=_capi.BACKPROP_REFERENCE, target_sync_interval=0,
                               mean_gradient=1, seed=0x5EED, first_game_id=0, overlap_collect=1, collects_per_update=1)
        t = xq.Trainer(cfg)
        t.set_td_bootstrap("legal")                  # (before the first collect: the ring records the side to move in s')
        t.dqn.set_optimizer("adam")
        t.dqn.set_td_loss("huber", 1.0)
        t.dqn.set_grad_clip(10.0)
        t.set_target_tau(0.01)
        t.set_reward(*RULE)
        t.set_opponent("random")
        t.set_colour_swap(prob)
        curve, done, train_s = [], 0, 0.0
        while True:
            t.synchronize()
            point = dict(colour_swap=prob, iterations=done, train_seconds=round(train_s, 2), **score(xq, t.dqn, args.pairs))
            point["training_versus"] = {k: (None if v != v else v) for k, v in t.versus_results().items()}     # (no game yet: no score)
            point["swap_calls"] = t.replay.colour_swap()[1]
            curve.append(point)
            print(json.dumps(point), flush=True)
            if done >= args.iters:
                break
            k = min(args.every, args.iters - done)
            t0 = time.perf_counter()
            t.step(k)
            t.synchronize()
            train_s += time.perf_counter() - t0
            done += k
        legs.append(dict(colour_swap=prob, curve=curve))
        t.close()
    with open(args.out, "w") as f:
        json.dump(dict(recipe=recipe, legs=legs), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
