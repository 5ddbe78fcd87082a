"""Negative control of the sparse-position inputs (not gpu): do they reject a subtly wrong move generator where the old ones do not?

tests/rules_restatement.py restates the DEVICE generator's structure in Python.  Unchanged it must reproduce the reference's lists
(ref_trace.npz, ref_sparse.npz) and the oracle's on the generated classes of tests/test_rules_sparse_gpu.py; with one seeded defect
the new inputs must tell.  Outcome, as run (a defect is "rejected" when some position's list or count differs):

    defect     ref_trace.npz alone   ref_sparse.npz   generated classes (a) (b) (c) (d)
    cannon1    rejected              rejected         rejected by (a), (b), (c)
    mirror0    rejected              rejected         rejected by (a), (b), (c)
    exit_m1    rejected              rejected         rejected by (a), (b), (c)
    exit_gt    not rejected          not rejected     not rejected — by NO input, see below

cannon1 and mirror0 are caught by random play too: 3 549 positions of dense middle games hold a cannon facing a lone piece and a
chariot or cannon whose backward ray ends on index 0.  What the new inputs add there is density (the line-stress class reaches the
defect on its first boards), not a first detection.

exit_gt — `pass * 8 > n_own` in place of `>=` — is an EQUIVALENT mutant of this generator: the early exit is an optimisation only.
With it wrong, a side of exactly 8 pieces (or of none) runs one more pass in which every lane fails `active = k < n_own` and emits
nothing, so the lists are the same for every board: the condition "each defect must be rejected" CANNOT be met for this one, by
these inputs or by any.  The test states that: it holds the mutant to equality on sides of 0, 8 and 16
pieces of every input instead of claiming a rejection no input can deliver.  So that the early-exit region keeps a control that
bites, a neighbouring real defect stands beside it: exit_m1, `pass * 8 >= n_own - 1`, loses the moves of a lone piece and of the
ninth of nine.  ref_trace.npz holds sides of nine pieces and rejects it too; a lone piece it never shows.
"""
import os

import numpy as np
import pytest

import rules_restatement as rr
import xqoracle as xo
from sparse_boards import gen_arbitrary, gen_endgames, gen_line_stress

OLD_TRACE_REJECTS = {"cannon1": True, "mirror0": True, "exit_m1": True, "exit_gt": False}


def _fixture_cases(golden_dir, name, stride=1):
    t = np.load(os.path.join(golden_dir, name))
    for i in range(0, len(t["board"]), stride):
        for colour, key in ((0, "red"), (1, "black")):
            yield t["board"][i], colour, t[key][t[key + "_off"][i]:t[key + "_off"][i + 1]].tolist()


def _oracle_cases(boards):
    for b in boards:
        ob = xo.board_from(b)
        for colour in (0, 1):
            codes, n = xo.all_valid_actions(ob, colour)
            yield b, colour, codes.tolist()


def _classes():
    return {"a": gen_endgames(1500, 0xE17D)[0], "b": gen_line_stress(0x11E5)[0][::41], "c": gen_arbitrary(1500, 0xA2B1)[0],
            "d": gen_arbitrary(300, 0xD00D, empty_mover=True)[0]}


def _rejects(cases, defect, only=None):
    """-> True at the first case whose list differs under the defect"""
    for board, colour, want in cases:
        if only is not None and int(((board > 0) & ((board > 7) == (colour == 1))).sum()) not in only:
            continue
        got, n = rr.gen_all_actions(board.tolist(), colour, defect)
        if got != want or n != len(want):
            return True
    return False


def test_restatement_without_a_defect_matches_reference_and_oracle(golden_dir):
    assert not _rejects(_fixture_cases(golden_dir, "ref_sparse.npz"), None)
    assert not _rejects(_fixture_cases(golden_dir, "ref_trace.npz", stride=5), None)
    assert not _rejects(_fixture_cases(golden_dir, "ref_bigmoves.npz", stride=4), None)
    for name, boards in _classes().items():
        assert not _rejects(_oracle_cases(boards), None), name


@pytest.mark.parametrize("defect", ["cannon1", "mirror0", "exit_m1"])
def test_seeded_defect_is_rejected_by_the_new_inputs(golden_dir, defect):
    assert _rejects(_fixture_cases(golden_dir, "ref_sparse.npz"), defect)
    by_class = {name: _rejects(_oracle_cases(boards), defect) for name, boards in _classes().items()}
    assert by_class["a"] and by_class["b"] and by_class["c"], by_class         # (d) holds one side only: not asked to tell
    assert _rejects(_fixture_cases(golden_dir, "ref_trace.npz"), defect) == OLD_TRACE_REJECTS[defect]
    if defect == "exit_m1":                                  # the lone piece is the new inputs' alone
        assert _rejects(_fixture_cases(golden_dir, "ref_sparse.npz"), defect, only=(1,))
        assert not _rejects(_fixture_cases(golden_dir, "ref_trace.npz"), defect, only=(1, 2, 3))


def test_early_exit_comparison_is_an_equivalent_mutant(golden_dir):
    """See the module docstring: no input can reject `pass * 8 > n_own`; sides of 0, 8 and 16 pieces are where it would show."""
    at = (0, 8, 16)
    assert not _rejects(_fixture_cases(golden_dir, "ref_sparse.npz"), "exit_gt")
    assert not _rejects(_fixture_cases(golden_dir, "ref_trace.npz"), "exit_gt", only=at) and not OLD_TRACE_REJECTS["exit_gt"]
    for name, boards in _classes().items():
        assert not _rejects(_oracle_cases(boards), "exit_gt", only=at), name
    n8 = sum(1 for b, c, _ in _fixture_cases(golden_dir, "ref_sparse.npz") if int(((b > 0) & ((b > 7) == (c == 1))).sum()) == 8)
    assert n8 >= 16                                          # the fixture does hold sides of exactly 8 pieces
