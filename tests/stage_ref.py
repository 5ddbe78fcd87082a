"""The staging pipeline of a TD step from a ring (DESIGN.md §4 "Staging pipeline") as the composition of the references of its stages,
in the pipeline's order: nstep_ref (assembly), mirror_ref, colour_swap_ref, view_ref.  No rule of its own: the slot columns are the
assembly's first and last slot (both the sampled slot without it), the side bytes follow colour_swap_ref (flipped on the flagged
rows) and view_ref (0 on every row), and the flags of s and s' under the view are the ring's mover column at the first slot and its
next_player column at the last."""
import numpy as np

import colour_swap_ref as cr
import mirror_ref as mr
import nstep_ref as nr
import view_ref as vr

ORDER = ("mirror", "colour_swap")


def stage(fx, slots, seed, gamma, n_step=1, mirror=0.0, colour_swap=0.0, view=False, legal=False, calls=(0, 0), order=ORDER):
    """The batch xq_dqn_td_grads_replay stages from ring contents fx (S, A, R, D, S2 by slot, cap, stride; mover and next_player
    columns where view or legal ask for them; size / write_pos when the ring is not exactly full) for the sampled `slots`.
    seed: the ring's; calls: the (mirror, colour swap) launch counts so far; order: of the two random transforms (they commute).
    -> dict(boards, next_boards, action, reward, done, slot, first_slot, last_slot, nstep (nstep_ref.assemble's dict or None),
            mirror_flags, colour_swap_flags, flag_s, flag_next (None for a stage that is off), next_player (None unless legal))"""
    if view and colour_swap > 0:
        raise ValueError("view and colour_swap exclude each other (xq_dqn_td_grads_replay refuses the pair)")
    slots = np.asarray(slots, np.int32)
    cap = fx["cap"]
    S, A, R, D, S2 = fx["S"][slots], fx["A"][slots], fx["R"][slots], fx["D"][slots], fx["S2"][slots]
    first = last = slots
    ref = None
    if n_step > 1:
        lo, count = nr.readable(cap, fx.get("size", cap), fx.get("write_pos", 0))
        ref = nr.assemble(fx["A"], fx["R"], fx["D"], cap, slots, n_step, fx["stride"], gamma, lo, count)
        S, A, R, D, S2 = nr.staged(fx, ref)
        first, last = ref["first_slot"], ref["last_slot"]
    side = np.asarray(fx["next_player"], np.uint8)[last] if legal else None
    out = dict(mirror_flags=None, colour_swap_flags=None, flag_s=None, flag_next=None)
    for name in order:
        if name == "mirror" and mirror > 0:
            m = mr.apply(S, A, S2, mirror, calls[0], seed)
            S, A, S2, out["mirror_flags"] = m["boards"], m["action"], m["next_boards"], m["flags"]
        if name == "colour_swap" and colour_swap > 0:
            c = cr.apply(S, A, S2, side, colour_swap, calls[1], seed)
            S, A, S2, out["colour_swap_flags"] = c["boards"], c["action"], c["next_boards"], c["flags"]
            side = c.get("next_player")
    if view:
        v = vr.apply(S, A, S2, np.asarray(fx["mover"])[first], np.asarray(fx["next_player"])[last])
        S, A, S2, out["flag_s"], out["flag_next"] = v["boards"], v["action"], v["next_boards"], v["flag_s"], v["flag_next"]
        if legal:
            side = v["next_player"]
    out.update(boards=S, next_boards=S2, action=np.asarray(A, np.int32), reward=np.asarray(R, np.float32), done=np.asarray(D, np.uint8),
               slot=slots, first_slot=np.asarray(first, np.int32), last_slot=np.asarray(last, np.int32), nstep=ref, next_player=side)
    return out
