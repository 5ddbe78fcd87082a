"""Definition of the zero-sum (negamax) TD target for self-play (xq_dqn_set_zero_sum, DESIGN.md §4 "Zero-sum target"), written out.
Test infrastructure only, like batch_ref.py: tests import it, the product path never does.

In a self-play transition (s, a, r, s') the side to move in s' is the OPPONENT of the mover of s, and every value the net gives for s'
is the opponent's.  What is good for the opponent is bad for the mover, so the opponent's best value is SUBTRACTED:

    1-step     y = done ? r : r - gamma * tanh(zm)
    n-step     R = r_0 - g r_1 + g^2 r_2 - ... : disc_k = (-1)^k g^k in the fp32 chain of tests/nstep_ref.py,
               y = done ? R : R + disc_n * tanh(zm)
    no move    (legal-move bootstrap) the side to move in s' has no move: it has lost, its value is -1, the lowest the net can express
               (tanh of the maximum over an empty list, -inf): y = r - gamma * (-1) = r + gamma

zm is what the handle's bootstrap, td_net and precision make it: everything that is not the sign comes from batch_ref.py (Q(s,a), the
activations, the forward operands), legal_ref.py (move lists, the winner, the candidate sets), nstep_ref.py (which slots a chain walks)
and huber_ref.py.  Nothing here negates an argument of those modules: tests/test_zero_sum_ref_cpu.py shows that the written-out rule
EQUALS them called with -gamma, and that the `+` rule does not.
"""
import numpy as np

import batch_ref as br
import legal_ref as lr
import nstep_ref as nr

NO_MOVE_VALUE = -1.0                 # tanh(-inf): the value of a side that cannot move


def target(R, D, t_next, gamma):
    """the rule itself on arrays: R rewards of the mover of s, D done, t_next = tanh(zm) the best value of the side to move in s'"""
    R = np.asarray(R, dtype=np.float64)
    return np.where(np.asarray(D).astype(bool), R, R - gamma * np.asarray(t_next, dtype=np.float64))


def forward(net, boards, next_boards, A, R, D, gamma, td_rule, precision=br.PRECISION_F32, target_net=None, chunk=br.CHUNK):
    """batch_ref.forward with the zero-sum target: a batch_ref.Forward whose y is r - gamma tanh(zm) (td_rule 0: the online net's maximum
    over all outputs, 1: the target net's, 2: Double DQN) and whose cand_y (Double DQN) are the zero-sum targets of the near-maximal
    online outputs.  Q(s,a), the activations and `live` are batch_ref's."""
    n = len(br._inputs(boards))
    f = br.forward(net, boards, next_boards, A, R, np.ones(n, bool), gamma, 0, precision)        # every row terminal: y = r, no s' pass
    D = np.asarray(D).reshape(n).astype(bool)
    f.D, f.td_rule = D, td_rule
    tnet = target_net if target_net is not None else net
    nb = br._inputs(next_boards)
    margin = br.CAND_MARGIN[precision]
    f.tanh_zm = np.zeros(n)
    for c0 in range(0, n, chunk):
        rows = c0 + np.nonzero(~D[c0:c0 + chunk])[0]
        if len(rows) == 0:
            continue
        x2 = br.one_hot(nb[rows])
        zn = net.z_out(net.hidden(x2)[-1]) if td_rule in (0, 2) else None
        zt = tnet.z_out(tnet.hidden(x2)[-1]) if td_rule in (1, 2) else None
        sel = zt if td_rule == 1 else zn
        val = zn if td_rule == 0 else zt
        star = np.argmax(sel, axis=1)                                   # first maximum
        k = np.arange(len(rows))
        f.astar[rows] = star
        f.tanh_zm[rows] = np.tanh(val[k, star])
        f.y[rows] = f.R[rows] - gamma * f.tanh_zm[rows]
        if td_rule == 2:
            zmax = sel[k, star]
            for j, i in enumerate(rows):
                cand = np.nonzero(sel[j] >= zmax[j] - margin)[0]
                f.cand_y[i] = f.R[i] - gamma * np.tanh(zt[j, cand])
    return f


def legal_forward(net, boards, next_boards, A, R, D, side, gamma, td_rule=0, target_net=None, precision=br.PRECISION_F32, lists=None):
    """legal_ref.forward with the zero-sum target: move lists, the winner a*, n_moves, zmax, z96 and the candidate sets are legal_ref's
    (the selection does not depend on the sign); y = r - gamma tanh(z_eval[a*]) on rows with a move, r + gamma on live, not-done rows
    whose side to move has none (zmax = -inf there, as the device reports it), r on done rows."""
    f = lr.forward(net, boards, next_boards, A, R, D, side, gamma, td_rule, target=target_net, precision=precision, lists=lists)
    ev = net if td_rule == 0 else target_net
    ze = lr.z96(ev, next_boards)
    f.y = f.R.copy()
    f.no_move = f.n_moves == 0
    for i in range(f.n):
        if f.n_moves[i] > 0:
            f.y[i] = f.R[i] - gamma * np.tanh(ze[i, f.astar[i]])
            f.cand_y[i] = f.R[i] - gamma * np.tanh(ze[i, f.cands[i]])
        elif f.n_moves[i] == 0:
            f.y[i] = f.R[i] - gamma * NO_MOVE_VALUE
            f.zmax[i] = -np.inf
            f.cand_y[i] = np.array([f.y[i]])
    return f


def discounts(gamma, n):
    """disc_0 = 1, disc_k = (-1)^k |disc_k| with |disc_k| = fl32(|disc_{k-1}| * (float)gamma), k = 0..n: the magnitudes of
    nstep_ref.discounts, the sign of the side whose reward the k-th slot of a self-play chain holds"""
    gf = np.float32(gamma)
    mag = [np.float32(1.0)]
    for _ in range(n):
        mag.append(np.float32(mag[-1] * gf))
    return [m if k % 2 == 0 else np.float32(-m) for k, m in enumerate(mag)]


def assemble(A, R, D, cap, slots, n, stride, gamma, first, count):
    """nstep_ref.assemble with the negamax return.  Which slots a chain walks, where it stops, what is dead and which next board is
    staged do not depend on the sign and are nstep_ref's; the reward is written out here: the mover's own rewards (even k) are added,
    the opponent's (odd k) subtracted, R = fl32(R + fl32(disc_k * r_k)) over the `steps` slots the chain used."""
    out = nr.assemble(A, R, D, cap, slots, n, stride, gamma, first, count)
    disc = discounts(gamma, n)
    rew = np.empty(len(out["reward"]), np.float32)
    for i, s in enumerate(np.asarray(slots)):
        s = int(s)
        off0 = (s - first) % cap
        Rn = np.float32(R[s])
        for k in range(1, int(out["steps"][i])):
            slot = (first + off0 + k * stride) % cap
            Rn = np.float32(Rn + np.float32(disc[k] * np.float32(R[slot])))
        rew[i] = Rn
    out["reward"] = rew
    return out


def n_step_target(Rn, Dn, t_next, gamma, n):
    """the target of an assembled row: y = done ? R : R + disc_n tanh(zm) — for odd n the side to move in the staged s' is the opponent
    (minus), for even n the mover again (plus)"""
    d = float(discounts(gamma, n)[n])
    Rn = np.asarray(Rn, dtype=np.float64)
    return np.where(np.asarray(Dn).astype(bool), Rn, Rn + d * np.asarray(t_next, dtype=np.float64))
