"""The hot-row table of cn_chess_ai_amd/csrc/xq_l0hot.h as the library builds it, read from tests/cpp/l0hot_probe.cpp (plain g++, no GPU)."""
import functools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
SRC = os.path.join(ROOT, "tests", "cpp", "l0hot_probe.cpp")
NO_ROW, COLD_BIT = 0xFFFF, 0x8000


@functools.lru_cache(maxsize=None)
def load_table():
    """{array name: values} + the scalars of the probe's head line"""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "l0hot_probe")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", SRC, "-o", exe])
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    t = {ln.split()[0]: np.array([int(x) for x in ln.split()[1:]]) for ln in out}
    ok, n_hot, n_cold, groups, group_rows, sq_b = (int(x) for x in t["head"])
    assert ok == 1
    t.update(n_hot=n_hot, n_cold=n_cold, groups=groups, group_rows=group_rows, sq_b=sq_b)
    return t


def hot_mask_rows(t):
    """bool [1260]: row is hot"""
    m = np.zeros(1260, bool)
    m[t["row"][t["row"] != NO_ROW]] = True
    return m
