#!/usr/bin/env python3
"""TEST INFRASTRUCTURE — regenerates tests/golden/*.npz from the REAL reference rules engine.

Runs only in the authoring container (needs /root/reference + conda QtCore): `make -C oracle ref` builds
oracle/_ref/xqref from /root/reference/src/chessboard.cpp unmodified, this script runs it and stores the
OUTPUTS (boards, ordered move lists, move results) as compact fixtures.  No reference source is copied.

    python oracle/gen_golden.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import xqoracle as xo  # noqa: E402

GOLD = os.path.join(os.path.dirname(HERE), "tests", "golden")


def run_trace(seed, ngames):
    with tempfile.NamedTemporaryFile(suffix=".bin") as f:
        subprocess.check_call([xo.REF_BIN, "trace", str(seed), str(ngames), f.name])
        return np.fromfile(f.name, dtype=xo.REF_RECORD)


def run_validmat(seed, npos):
    with tempfile.NamedTemporaryFile(suffix=".bin") as f:
        subprocess.check_call([xo.REF_BIN, "validmat", str(seed), str(npos), f.name])
        raw = np.fromfile(f.name, dtype=np.uint8).reshape(npos, 90 + 8100)
    return raw[:, :90].copy(), np.packbits(raw[:, 90:], axis=1)


def run_tracebig(seed, nrec):
    with tempfile.NamedTemporaryFile(suffix=".bin") as f:
        subprocess.check_call([xo.REF_BIN, "tracebig", str(seed), str(nrec), f.name])
        return np.fromfile(f.name, dtype=xo.REF_RECORD)


def run_rulemat(seed, npos):
    with tempfile.NamedTemporaryFile(suffix=".bin") as f:
        subprocess.check_call([xo.REF_BIN, "rulemat", str(seed), str(npos), f.name])
        raw = np.fromfile(f.name, dtype=np.uint8).reshape(npos, 90 + 7 * 8100 + 64 * 6)
    q = raw[:, 90 + 7 * 8100:].reshape(npos, 64, 6).view(np.int8)
    return raw[:, :90].copy(), np.packbits(raw[:, 90:90 + 7 * 8100], axis=1), q[:, :, :5].copy(), q[:, :, 5].astype(np.uint8)


def run_sparse(seed, ngames):
    with tempfile.NamedTemporaryFile(suffix=".bin") as f, tempfile.NamedTemporaryFile(suffix=".bin") as fm:
        subprocess.check_call([xo.REF_BIN, "sparse", str(seed), str(ngames), f.name, fm.name])
        rec = np.fromfile(f.name, dtype=xo.REF_RECORD)
        raw = np.fromfile(fm.name, dtype=np.uint8).reshape(-1, 90 + 8 * 8100)
    return rec, raw[:, :90].copy(), raw[:, 90:90 + 8100].copy(), raw[:, 90 + 8100:].copy()


def side_counts(boards):
    return ((boards >= 1) & (boards <= 7)).sum(axis=1), (boards >= 8).sum(axis=1)


def far_soldiers(boards):
    """(a red soldier stands on row 9, a black soldier stands on row 0)"""
    return (boards[:, 81:] == 7).any(axis=1), (boards[:, :9] == 14).any(axis=1)


def select_sparse(rec):
    """Deduplicates the steered records by (board, side to move) and keeps, in play order, each record that still fills one of the
    quotas below — the regions tests/test_oracle_golden.py::test_sparse_fixture_covers_the_thin_regions asks for, with headroom.
    -> indices into rec."""
    b = rec["board"]
    nr, nb = side_counts(b)
    fr, fb = far_soldiers(b)
    missing = ~(b == 1).any(axis=1) | ~(b == 8).any(axis=1)
    walked = ((b == 1).any(axis=1) & (b[:, 4] != 1)) | ((b == 8).any(axis=1) & (b[:, 85] != 8))
    quota = {}
    for k in range(17):
        quota["red", k] = quota["black", k] = 20
    quota.update(far_both=48, far_red=24, far_black=24, missing=96, zero_red=12, zero_black=12, invalid=24, walked=32,
                 tiny=160, general_taken=24)
    seen, keep = set(), []
    for i in range(len(rec)):
        key = b[i].tobytes() + bytes([rec["player"][i]])
        if key in seen:
            continue
        tags = [("red", int(nr[i])), ("black", int(nb[i]))]
        if fr[i] and fb[i]: tags.append("far_both")
        if fr[i]: tags.append("far_red")
        if fb[i]: tags.append("far_black")
        if missing[i]: tags.append("missing")
        if rec["nRed"][i] == 0: tags.append("zero_red")
        if rec["nBlack"][i] == 0: tags.append("zero_black")
        if not rec["valid"][i]: tags.append("invalid")
        if walked[i]: tags.append("walked")
        if nr[i] + nb[i] <= 6: tags.append("tiny")             # few enough pieces for a depth-3 search on the CPU
        if rec["captured"][i] in (1, 8): tags.append("general_taken")
        if any(quota[t] > 0 for t in tags):
            for t in tags:
                quota[t] -= 1
            seen.add(key)
            keep.append(i)
    return np.array(keep)


def sparse_extras(rec, keep, mboard, mvalid, mrule):
    """-> (after_board, after_meta of the kept records; the arrays of ref_sparse_mat.npz)"""
    # the state after a valid attempt i is the snapshot of record i + 1 (every game ends with a record whose attempt is off the
    # board); an invalid attempt changes nothing
    assert not rec["valid"][-1]
    nxt = np.where(rec["valid"] != 0, np.minimum(np.arange(len(rec)) + 1, len(rec) - 1), np.arange(len(rec)))
    after_board = rec["board"][nxt]
    after_meta = np.stack([rec[k][nxt] for k in ("moveCount", "player", "redScore", "blackScore")], axis=1).astype(np.int32)
    # matrices: deduplicated, the small positions first
    nr, nb = side_counts(mboard)
    fr, fb = far_soldiers(mboard)
    quota = dict(small=28, far=12, other=8)
    seen, mk = set(), []
    for i in range(len(mboard)):
        key = mboard[i].tobytes()
        tag = "small" if min(nr[i], nb[i]) <= 3 else ("far" if fr[i] or fb[i] else "other")
        if key in seen or quota[tag] <= 0:
            continue
        quota[tag] -= 1
        seen.add(key)
        mk.append(i)
    mk = np.array(mk)
    mats = dict(board=mboard[mk], valid_bits=np.packbits(mvalid[mk], axis=1), rule_bits=np.packbits(mrule[mk], axis=1))
    return after_board[keep], after_meta[keep], mats


def save_sparse(rec, keep, mboard, mvalid, mrule):
    after_board, after_meta, mats = sparse_extras(rec, keep, mboard, mvalid, mrule)
    save_trace("ref_sparse.npz", rec[keep], after_board=after_board, after_meta=after_meta)
    np.savez_compressed(os.path.join(GOLD, "ref_sparse_mat.npz"), **mats)
    return len(mats["board"])


SPARSE_SEED, SPARSE_GAMES = 0x5BA55E, 48


def save_trace(name, rec, **extra):
    # ragged move lists -> flat arrays + offsets (keeps the fixture small)
    def flat(field, nfield):
        n = rec[nfield].astype(np.int64)
        assert n.max() <= 128
        off = np.concatenate([[0], np.cumsum(n)])
        out = np.concatenate([rec[field][i, :n[i]] for i in range(len(rec))]).astype(np.uint16)
        return out, off.astype(np.int32)
    red, red_off = flat("red", "nRed")
    black, black_off = flat("black", "nBlack")
    np.savez_compressed(
        os.path.join(GOLD, name),
        board=rec["board"], moveCount=rec["moveCount"], player=rec["player"], redScore=rec["redScore"],
        blackScore=rec["blackScore"], over=rec["over"], winner=rec["winner"],
        red=red, red_off=red_off, black=black, black_off=black_off,
        move=np.stack([rec["fr"], rec["fc"], rec["tr"], rec["tc"]], axis=1), valid=rec["valid"],
        captured=rec["captured"], **extra)


def main():
    subprocess.check_call(["make", "-s", "-C", HERE, "ref"])
    os.makedirs(GOLD, exist_ok=True)
    sp, mboard, mvalid, mrule = run_sparse(SPARSE_SEED, SPARSE_GAMES)     # steered play: bare endgames, far-rank soldiers, fallen generals
    keep = select_sparse(sp)
    nmat = save_sparse(sp, keep, mboard, mvalid, mrule)
    print("sparse records:", len(keep), "of", len(sp), "| matrix positions:", nmat, "of", len(mboard))
    big = run_tracebig(0xB16, 160)           # positions where a side has > 64 moves (second half of the 128-entry lists)
    save_trace("ref_bigmoves.npz", big)
    print("bigmoves records:", len(big), "max moves:", int(max(big["nRed"].max(), big["nBlack"].max())))
    rb, rbits, rq, rres = run_rulemat(0xFACE, 24)
    np.savez_compressed(os.path.join(GOLD, "ref_rulemat.npz"), board=rb, rule_bits=rbits, query=rq, query_result=rres)
    print("rulemat positions:", len(rb), "queries true:", int(rres.sum()), "of", rres.size)
    live = run_trace(12345, 6)               # the run tests/test_oracle_golden.py::test_live_cross_check_against_reference_binary repeats
    save_trace("ref_trace_live.npz", live)
    print("live trace records:", len(live))
    rec = run_trace(0x5EED, 20)
    def flat(field, nfield):
        n = rec[nfield].astype(np.int64)
        assert n.max() <= 128
        off = np.concatenate([[0], np.cumsum(n)])
        out = np.concatenate([rec[field][i, :n[i]] for i in range(len(rec))]).astype(np.uint16)
        return out, off.astype(np.int32)
    red, red_off = flat("red", "nRed")
    black, black_off = flat("black", "nBlack")
    np.savez_compressed(
        os.path.join(GOLD, "ref_trace.npz"),
        board=rec["board"], moveCount=rec["moveCount"], player=rec["player"], redScore=rec["redScore"],
        blackScore=rec["blackScore"], over=rec["over"], winner=rec["winner"],
        red=red, red_off=red_off, black=black, black_off=black_off,
        move=np.stack([rec["fr"], rec["fc"], rec["tr"], rec["tc"]], axis=1), valid=rec["valid"],
        captured=rec["captured"])
    boards, mats = run_validmat(0xC0FFEE, 64)
    np.savez_compressed(os.path.join(GOLD, "ref_validmat.npz"), board=boards, valid_bits=mats)
    print("records:", len(rec), "positions with both-side lists; max moves:",
          int(max(rec["nRed"].max(), rec["nBlack"].max())),
          "| validmat positions:", len(boards))
    for f in sorted(os.listdir(GOLD)):
        print(f, os.path.getsize(os.path.join(GOLD, f)))


if __name__ == "__main__":
    main()
