"""The device move generator (gen_all_actions / ray_scan / bits_at of cn_chess_ai_amd/csrc/xq_rules.hip.h) restated in Python, with
four switchable defects — the negative control of tests/test_rules_negative_control_cpu.py.

The restatement keeps the kernel's structure, not the reference's: own pieces ranked by square into a 16-entry table, two passes
of eight pieces with the early exit between them, eight direction slots per piece, chariot and cannon rays resolved by bit scans
on a 9-bit row / 10-bit column occupancy (a backward ray = the forward ray of the mirrored line, indices mirrored back), the
128-entry list clipped once per slot.

DEFECTS
    "exit_gt"  the early exit reads `pass * 8 > n_own` in place of `>=`
    "exit_m1"  the early exit is taken one piece early: `pass * 8 >= n_own - 1` (a ninth piece is never reached)
    "cannon1"  a cannon captures the FIRST piece on its ray when nothing stands behind it
    "mirror0"  a backward ray's hit is not mirrored back when it lies on index 0 of the line
"""
MAX_MOVES = 128
DEFECTS = ("exit_gt", "exit_m1", "cannon1", "mirror0")


def _ctz(x):
    return (x & -x).bit_length() - 1


def ray_scan(line, pos, length, forward, defect=None):
    """-> (empties, first, second) as RayHit"""
    if forward:
        l, p = line, pos
    else:
        l = int(format(line, "0%db" % length)[::-1], 2)
        p = length - 1 - pos
    x = l >> (p + 1)
    if x == 0:
        return length - 1 - p, -1, -1
    e = _ctz(x)
    y = x >> (e + 1)
    first = p + 1 + e
    second = p + 2 + e + _ctz(y) if y else -1

    def back(i):
        if i < 0 or forward:
            return i
        if defect == "mirror0" and i == length - 1:
            return i
        return length - 1 - i
    return e, back(first), back(second)


def gen_all_actions(sq, player, defect=None):
    """-> (codes clipped to MAX_MOVES, count clipped to MAX_MOVES); sq = 90 piece codes."""
    black = player == 1
    own = [s for s in range(90) if sq[s] and (sq[s] > 7) == black]
    n_own = len(own)
    rank_sq = own[:16]
    moves, total = [], 0

    def put(code):
        if len(moves) < MAX_MOVES:
            moves.append(code)

    for ps in range(2):
        if defect == "exit_gt":
            leave = ps * 8 > n_own
        elif defect == "exit_m1":
            leave = ps * 8 >= n_own - 1
        else:
            leave = ps * 8 >= n_own
        if leave:
            break
        for k in range(ps * 8, ps * 8 + 8):
            if not k < n_own:                                   # `active`
                continue
            frm = rank_sq[k]
            p = sq[frm]
            row, col = divmod(frm, 9)
            t = p - 7 if p > 7 else p
            fw = -1 if black else 1
            crossed = row < 5 if black else row > 4
            for slot in range(8):
                lt4, lt2 = slot < 4, slot < 2
                sg1 = -1 if slot & 1 else 1
                sg2 = -1 if slot & 2 else 1
                if t in (5, 6):
                    if not lt4:
                        continue
                    horiz, fwd = lt2, (slot & 1) == 0
                    if horiz:
                        line = sum(1 << c for c in range(9) if sq[row * 9 + c])
                        pos, length = col, 9
                    else:
                        line = sum(1 << r for r in range(10) if sq[r * 9 + col])
                        pos, length = row, 10
                    empties, first, second = ray_scan(line, pos, length, fwd, defect)
                    delta = (1 if fwd else -1) if horiz else (9 if fwd else -9)
                    hit = first if t == 5 else second
                    if t == 6 and defect == "cannon1" and second < 0:
                        hit = first
                    n_run, extra = empties, -1
                    if hit >= 0:
                        bs = row * 9 + hit if horiz else hit * 9 + col
                        if (sq[bs] > 7) != black:
                            if t == 5:
                                n_run += 1
                            else:
                                extra = bs
                    for i in range(n_run):
                        put(frm * 90 + frm + delta * (i + 1))
                    if extra >= 0:
                        put(frm * 90 + extra)
                    total += n_run + (extra >= 0)
                    continue
                mag = 2 if t == 3 else 1
                dr, dc = (mag if lt2 else -mag), sg1 * mag
                if t == 1:
                    dr, dc = (sg1 if lt2 else 0), (0 if lt2 else sg1)
                if t == 4:
                    dr, dc = (sg2 if lt4 else 2 * sg2), (2 * sg1 if lt4 else sg1)
                if t == 7:
                    dr, dc = (fw if slot == 0 else 0), (-1 if slot == 1 else (1 if slot == 2 else 0))
                if t == 4:
                    slot_ok = True
                elif t == 7:
                    slot_ok = slot == 0 or (slot < 3 and crossed)
                else:
                    slot_ok = lt4
                nr, nc = row + dr, col + dc
                inside = 0 <= nr < 10 and 0 <= nc < 9
                pal_col = 3 <= nc <= 5
                if t == 1:
                    rule = (3 <= col <= 5 and (row <= 2 or row >= 7)) and pal_col and (nr <= 2 or nr >= 7)
                elif t == 2:
                    rule = pal_col and (nr >= 7 if black else nr <= 2)
                elif t == 3:
                    rule = (nr >= 5 if black else nr <= 4) and ((row < 5) == (nr < 5))
                else:
                    rule = True
                if not (slot_ok and inside and rule):
                    continue
                if t in (3, 4):
                    gr, gc = row + int(dr / 2), col + int(dc / 2)          # truncating /2
                    if sq[gr * 9 + gc]:
                        continue
                tp = sq[nr * 9 + nc]
                if tp == 0 or (tp > 7) != black:
                    put(frm * 90 + nr * 9 + nc)
                    total += 1
    return moves, min(total, MAX_MOVES)
