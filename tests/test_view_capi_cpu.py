"""The mover view's entry points (not gpu): include/xq_capi.h, the ctypes table, the library's exports and the Python and C++ surfaces
agree on them; the enum; the argument errors that need no device; the work model's two brackets; the facade probe and the example
compile with plain g++."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xq_capi.h")
NEW_SYMBOLS = ("xq_dqn_set_view", "xq_dqn_get_view", "xq_view_boards_dev", "xq_dqn_last_view", "xq_replay_track_mover",
               "xq_replay_push_host_sides", "xq_replay_get_mover", "xq_env_set_q_view", "xq_env_get_q_view", "xq_trainer_set_view",
               "xq_arena_ply_q_dev_view")


@pytest.fixture(scope="module")
def capi():
    lib = os.path.join(ROOT, "cn_chess_ai_amd", "libxqhip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "cn_chess_ai_amd", "csrc"), "all"])
    from cn_chess_ai_amd import _capi
    _capi.load()
    return _capi


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_view_symbols_are_declared_exported_and_bound(capi):
    declared = set(re.findall(r"\b(xq_[a-z0-9_]+)\s*\(", header_text()))
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    exported = set(re.findall(r" T (xq_[a-z0-9_]+)", out))
    lib = capi.load()
    for n in NEW_SYMBOLS:
        assert n in declared and n in exported and n in capi.PROTOTYPES and n in capi.LAZY_VIEW, n
        assert getattr(lib, n).argtypes == capi.PROTOTYPES[n]
    assert set(capi.LAZY_VIEW) == set(NEW_SYMBOLS)
    assert not set(capi.LAZY_VIEW) & (set(capi.LAZY_LEGAL) | set(capi.LAZY_COLOUR_SWAP) | set(capi.LAZY_ZERO_SUM))


def test_enum_and_prototypes_match_the_header(capi):
    text = header_text()
    assert re.search(r"enum\s*\{\s*XQ_VIEW_ABSOLUTE\s*=\s*0\s*,\s*XQ_VIEW_MOVER\s*=\s*1\s*\}", text)
    assert (capi.VIEW_ABSOLUTE, capi.VIEW_MOVER) == (0, 1)
    vp, i32, d = C.c_void_p, C.c_int32, C.c_double
    pi, pu8 = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    want = {"xq_dqn_set_view": ("xq_dqn* d, int view", [vp, i32]),
            "xq_dqn_get_view": ("const xq_dqn* d, int* view", [vp, pi]),
            "xq_view_boards_dev": ("const void* boards_dev, const void* side_dev, int n, void* out_dev, void* hip_stream", [vp, vp, i32, vp, vp]),
            "xq_dqn_last_view": ("xq_dqn* d, int n, uint8_t* flag_s, uint8_t* flag_next, uint8_t* boards90, uint8_t* next_boards90, "
                                 "int32_t* action_to, int32_t* slot", [vp, i32, pu8, pu8, pu8, pu8, pi, pi]),
            "xq_replay_track_mover": ("xq_replay* r", [vp]),
            "xq_replay_get_mover": ("xq_replay* r, int first, int n, uint8_t* out", [vp, i32, i32, pu8]),
            "xq_env_set_q_view": ("xq_env* e, int on", [vp, i32]),
            "xq_env_get_q_view": ("const xq_env* e, int* on", [vp, pi]),
            "xq_trainer_set_view": ("xq_trainer* t, int view", [vp, i32]),
            "xq_arena_ply_q_dev_view": ("xq_arena* a, const float* q_dev, int q_stride, double eps_a, double eps_b, int view_a, int view_b",
                                        [vp, vp, i32, d, d, i32, i32])}
    for name, (params, argtypes) in want.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m and " ".join(m.group(1).split()) == params, name
        assert capi.PROTOTYPES[name] == argtypes, name
    m = re.search(r"\bint\s+xq_replay_push_host_sides\s*\(([^)]*)\)\s*;", text)
    assert m and " ".join(m.group(1).split()).endswith("const uint8_t* mover, const uint8_t* next_player")
    assert len(capi.PROTOTYPES["xq_replay_push_host_sides"]) == 9


def test_view_on_a_null_handle_fails_loudly(capi):
    """no device is needed to be refused: a NULL handle or pointer is XQ_ERR_INVALID_ARGUMENT from every new entry point, with a message"""
    v = C.c_int32()
    b = (C.c_uint8 * 4)()
    calls = [("xq_dqn_set_view", (None, 1)), ("xq_dqn_get_view", (None, C.byref(v))), ("xq_dqn_last_view", (None, 1) + (None,) * 6),
             ("xq_replay_track_mover", (None,)), ("xq_replay_get_mover", (None, 0, 1, b)),
             ("xq_replay_push_host_sides", (None, 0) + (None,) * 7), ("xq_env_set_q_view", (None, 1)),
             ("xq_env_get_q_view", (None, C.byref(v))), ("xq_trainer_set_view", (None, 1)),
             ("xq_arena_ply_q_dev_view", (None, None, 96, 0.0, 0.0, 1, 0))]
    for name, args in calls:
        with pytest.raises(capi.XqError) as e:
            capi.call(name, *args)
        assert e.value.code == 1 and "null" in str(e.value).lower(), name
    # xq_view_boards_dev has no handle: its pointers, its count and the aliasing rule
    buf = C.cast(b, C.c_void_p)
    for args in ((None, buf, 1, buf, None), (buf, None, 1, buf, None), (buf, buf, 1, None, None), (buf, buf, -1, buf, None)):
        with pytest.raises(capi.XqError) as e:
            capi.call("xq_view_boards_dev", *args)
        assert e.value.code == 1 and "bad argument" in str(e.value)
    with pytest.raises(capi.XqError) as e:
        capi.call("xq_view_boards_dev", buf, buf, 1, buf, None)
    assert e.value.code == 1 and "must not be boards_dev" in str(e.value)


def test_python_surface_has_the_setters():
    import cn_chess_ai_amd as m
    from cn_chess_ai_amd import dqn, vecenv
    for cls, names in ((dqn.DQN, ("set_view", "view", "last_view")), (dqn.Trainer, ("set_view",)),
                       (vecenv.ReplayBuffer, ("track_mover", "mover")), (vecenv.VecEnv, ("set_q_view",))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
    assert callable(m.view_boards) and "view_boards" in m.__all__
    assert dqn.VIEWS == {"absolute": 0, "mover": 1}


def test_work_model_knows_the_two_view_brackets_only_when_asked():
    import cn_chess_ai_amd.workmodel as wm
    cfg = ((1260, 256, 256, 8100), 8192, 8192)
    base, same, on = wm.step_work(*cfg), wm.step_work(*cfg, view=False), wm.step_work(*cfg, view=True)
    assert base == same and "mover_view_stage" not in base and "view_boards@select" not in base
    assert set(on) - set(base) == {"mover_view_stage", "view_boards@select"} and all(on[k] == base[k] for k in base)
    assert on["mover_view_stage"]["hbm_bytes"] == 8192 * 218 and on["view_boards@select"]["hbm_bytes"] == 8192 * 112
    for other in (dict(n_step=3), dict(mirror=True), dict(n_step=3, mirror=True)):
        off, both = wm.step_work(*cfg, **other), wm.step_work(*cfg, view=True, **other)
        assert set(both) - set(off) == {"mover_view_stage", "view_boards@select"} and all(both[k] == off[k] for k in off), other
        assert both["mover_view_stage"]["hbm_bytes"] == 8192 * 212
    per = wm.step_work(*cfg, prioritized=True, view=True)
    assert set(per) - set(wm.step_work(*cfg, prioritized=True)) == {"mover_view_stage", "view_boards@select", "per_writeback"}
    legal = wm.step_work(*cfg, bootstrap="legal", view=True)
    assert legal["mover_view_stage"]["hbm_bytes"] == 8192 * 219 and "legal_side_stage" not in legal
    lm, lm_on = wm.step_work(*cfg, bootstrap="legal", mirror=True), wm.step_work(*cfg, bootstrap="legal", mirror=True, view=True)
    assert "legal_side_stage" in lm and "legal_side_stage" not in lm_on
    with pytest.raises(ValueError):
        wm.step_work(*cfg, view=True, colour_swap=True)
    assert wm.rocprof_kernel("mover_view_stage", *cfg[:2]) == "mover_view_stage_kernel("
    assert wm.rocprof_kernel("view_boards@select", *cfg[:2]) == "view_boards_kernel("


def build_view_facade_probe():
    from test_arena_cpu import gxx, BUILD
    return gxx(os.path.join(ROOT, "tests", "cpp", "view_facade.cpp"), os.path.join(BUILD, "view_facade"))


def build_example():
    from test_arena_cpu import gxx, BUILD
    return gxx(os.path.join(ROOT, "examples", "train_selfplay.cpp"), os.path.join(BUILD, "train_selfplay_view"))


def test_view_facade_probe_and_example_compile(capi):
    """xq::View, xq::DQN::setView / view, xq::ChessAI::setView / view and TrainStats::view with plain g++ (no HIP headers)"""
    assert os.path.exists(build_view_facade_probe())
    exe = build_example()
    out = subprocess.run([exe, "1", "m.bin", "1", "view=sideways"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "view=" in out.stderr
