"""Kernel time of the apply with and without the soft target update at 8192 x 256^2, from the handle's own kernel-exact events
(xq_dqn_kernel_stats): tau = 0, tau = 0.01 with the target in step outside the TD segments (the update rides in the apply kernel) and
tau = 0.01 after set_params(target) (the plain apply + soft_target_kernel), under SGD and Adam, each leg twice.  Prints one JSON object;
profiles/NOTES.md ("Soft target update") says what to set the figures against.

    python tools/soft_target_time.py [--steps 40]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    args = ap.parse_args()
    import cn_chess_ai_amd as xq
    from test_dqn_gpu import CFG2_NET, make_net
    from test_td_full_size_gpu import selfplay_batch
    n = 8192
    S, A, R, D, S2 = selfplay_batch(xq, n, seed=77, plies=25, every=9)
    out = {}
    for opt in ("sgd", "adam"):
        for name, tau, in_step in (("tau0", 0.0, True), ("fused", 0.01, True), ("whole", 0.01, False), ("tau0_again", 0.0, True),
                                   ("fused_again", 0.01, True)):
            d, _, _ = make_net(xq, CFG2_NET, seed=5)
            d.set_optimizer(opt)
            d.set_fused_apply(True)
            if not in_step:
                d.set_params(*d.get_params(1), net=1)
            d.set_target_tau(tau)
            rp = xq.ReplayBuffer(n, seed=1)
            rp.push(S, A, R, D, S2)
            for _ in range(2):                                   # the first round warms up
                d.kernel_stats(2)
                for _ in range(args.steps):
                    rp.sample(n)
                    d.td_grads_replay(rp, n, td_net=0, mode=0)
                    d.apply_grads(1e-3, 1.0 / n)
                st = {s["name"]: s for s in d.kernel_stats(0)}
            a = st["adam_apply" if opt == "adam" else "sgd_apply"]
            r = dict(apply_us=1e3 * a["ms"] / a["launches"], exact=a["exact"], launches=a["launches"])
            if "soft_target" in st:
                r["soft_target_us"] = 1e3 * st["soft_target"]["ms"] / st["soft_target"]["launches"]
            out[f"{opt}_{name}"] = r
            rp.close(); d.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
