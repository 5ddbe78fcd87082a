"""The trainer's ring windows as the device tests restate them, from the ring's (size, total) BEFORE the iteration's collects.  The library
states them once in cn_chess_ai_amd/csrc/xq_ring_window.h; tests/test_ring_window_cpu.py checks both against a simulated ring."""


def overlap_window(size, total, cap, m):
    """Eligible ring slots while a collect of m transitions is in flight: (start, count) from the pre-collect state."""
    w = total % cap
    if size + m < cap:
        return 0, size
    return (w + m) % cap, cap - m


def default_range(size, total, cap):
    return (0 if size < cap else total % cap), size


def tree_range(size, total, cap, G):
    """the readable range that goes with the tree learn_apply builds: the filled ring minus the next collect's slots once they wrap"""
    if size + G > cap:
        return (total % cap + G) % cap, cap - G
    return default_range(size, total, cap)
