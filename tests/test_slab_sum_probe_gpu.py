"""The ordered sums of xq_apply.hip.h bit for bit against plain C++ loops — `pytest -m gpu`.

tools/slab_sum_probe.hip includes the kernel header itself and runs reduce_slabs_kernel, sgd_segments_kernel (stepping and reduce_only),
adam_segments_kernel and colsum_partial_kernel over the slab counts, lengths, strides and alignments at which a batch boundary, a
leftover term or the scalar path can go wrong (the lists are in its header comment), against host loops that spell the order of additions.
Its host-only negative control fails it if the inputs of a shape could not tell the four-chain order from the ascending one.  This test
builds the probe, runs it once as a child process and expects no mismatch.
"""
import os
import re
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hipcc():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_slab_sum_probe(tmp_path):
    exe = str(tmp_path / "slab_sum_probe")
    # host half with contraction off (the references say std::fmaf where the device contracts); device half with the library's flags
    subprocess.run([hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-Xarch_host", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    "-o", exe, os.path.join(ROOT, "tools", "slab_sum_probe.hip")], check=True, timeout=300)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout[-4000:])
    m = re.search(r"^slab_sum_probe: mismatches (\d+)$", r.stdout, re.M)
    assert m is not None, "the probe did not report"
    assert int(m.group(1)) == 0
    assert re.search(r"control failures 0$", r.stdout, re.M), "the negative control did not hold"
    assert r.returncode == 0
