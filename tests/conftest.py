import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def golden():
    class G:
        def __getitem__(self, name):
            return np.load(os.path.join(GOLDEN, name))

        def json(self, name):
            import json
            return json.load(open(os.path.join(GOLDEN, name)))
    return G()


@pytest.fixture(scope="session")
def mips():
    from topsy_amd import kernel_lut
    return kernel_lut.kernel_mips()


def make_cloud(n, seed=0, h_scale=1.0):
    """Seeded test cloud with a wide range of smoothing lengths (sub-pixel ... several hundred px)."""
    rs = np.random.RandomState(seed)
    pos = (rs.normal(size=(n, 3)) * np.array([30.0, 20.0, 40.0])).astype(np.float32)
    h = (np.exp(rs.uniform(np.log(0.02), np.log(60.0), size=n)) * h_scale).astype(np.float32)
    m = rs.uniform(0.5, 2.0, size=n).astype(np.float32)
    q = rs.normal(size=n).astype(np.float32)
    rgb = rs.uniform(0.0, 1.0, size=(n, 3)).astype(np.float32)
    return pos, h, m, q, rgb


def spawn_ranks(fn, world, *args):
    """Run fn(rank, world, *args) in `world` fresh processes and wait for them (what torch.multiprocessing.spawn does: when
    one rank fails the others are stopped, so none is left waiting at a rendezvous).  torch must be imported by the workers
    only, never by the test process: once libtopsy_splat.so has brought up the system HIP runtime here, importing torch
    loads its bundled HIP runtime and RCCL beside it, the library's dlopen("librccl.so") then finds torch's copy, and that
    copy sees no device -- every later RCCL communicator of the session fails."""
    import multiprocessing
    from multiprocessing.connection import wait
    mp = multiprocessing.get_context("spawn")
    procs = [mp.Process(target=fn, args=(rank, world) + args) for rank in range(world)]
    for p in procs:
        p.start()
    try:
        pending = {p.sentinel: p for p in procs}      # (a sentinel stays readable once its process has ended)
        while pending and not any(p.exitcode for p in procs):
            for s in wait(list(pending)):
                pending.pop(s).join()
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
            p.join()
    codes = [p.exitcode for p in procs]
    assert codes == [0] * world, f"exit codes of ranks 0..{world - 1}: {codes}"
