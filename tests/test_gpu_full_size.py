"""Full-size parity of the BASELINE configurations, driver-run, each behind a resource probe (HBM + host memory) and nothing else:
tests/big_c3_check.py (weighted RMAT-24, p = .25 q = 4 at walkLength 80 over 20 000 sampled walkers, (4, .5), (.25, 1) over ~1 500, incl. the highest-degree starts, against
the CPU oracle over the rows of every vertex on their device paths, rebuilt on the host from the same edge stream), tests/big_c5_check.py
(config 5's stand-in, directed RMAT-26 ef 27, p = 4 q = .5, the same way) and tests/big_c4_check.py
(config 4 at its own size, RMAT-27, on eight virtual shards against the single-launch kernel — the distributed == sequential
property of T/UniformRandomWalkTest.scala:181-291 at size — and ~1 500 sampled walkers against the oracle over rows rebuilt on the
host from the edge stream) and tests/big_shard_tables_check.py (the sharded per-edge tables at config 3's size, worlds 1 and 2,
every walker against the replicated kernel), tests/big_every_walker_check.py (configs 3 and 5's stand-in: one
iteration at walkLength 80 through the default table path, the other table kernel and the on-the-fly samplers — ALL walkers compared;
run inside big_c3_check.py / big_c5_check.py with `every`, so each configuration builds its graph and tables once for both of its tests).  A box that lacks the memory FAILS these tests; only SRW_SKIP_FULL_SIZE=1 skips
them (quick local runs)."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(bool(os.environ.get("SRW_SKIP_FULL_SIZE")), reason="SRW_SKIP_FULL_SIZE is set")]


def _resources():
    import torch
    free, _ = torch.cuda.mem_get_info(0)
    host = os.sysconf("SC_PAGE_SIZE") * os.sysconf("SC_AVPHYS_PAGES")
    return free, host


def _need(free_gb, host_gb):
    """A resource shortfall is a failure, not a skip: a silently skipped full-size test would leave the suite green."""
    free, host = _resources()
    if free < free_gb * 1e9 or host < host_gb * 1e9:
        pytest.fail("needs ~%d GB of free HBM and ~%d GB of host memory (have %.0f / %.0f GB); SRW_SKIP_FULL_SIZE=1 skips the "
                    "full-size tests on purpose" % (free_gb, host_gb, free / 1e9, host / 1e9))


def _run(script, *args, timeout=3000, check=True):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", script), *args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=timeout, env=dict(os.environ, SRW_CHECK_QUICK="1"))      # parity only: the scripts' timing walks are skipped
    if check:
        assert r.returncode == 0 and "parity OK" in r.stdout, r.stdout[-3000:]
        assert "MISMATCH" not in r.stdout
    return r.returncode, r.stdout


def _part(run, tag, result):
    """The lines of one of the two checks a merged script ran (the oracle's or the every-walker one), which must have passed on its own."""
    rc, out = run
    assert (result + " parity OK") in out, out[-3000:]
    # the script must also have ended cleanly: no signal, and a non-zero status only when the OTHER check reported its failure
    assert rc >= 0, "killed by signal %d\n%s" % (-rc, out[-3000:])
    assert rc == 0 or "PARITY FAILED" in out, "exit status %d\n%s" % (rc, out[-3000:])
    lines = [ln for ln in out.splitlines() if tag in ln]
    assert not any("MISMATCH" in ln for ln in lines), out[-3000:]
    return lines


# configs 3 and 5: the oracle's sampled walkers and every walker through the other samplers come from ONE process (one graph, one table
# build, the same default walk); each test asserts its own half of the output
@pytest.fixture(scope="module")
def config3_run():
    _need(200, 24)
    return _run("big_c3_check.py", "every", check=False)


@pytest.fixture(scope="module")
def config5_run():
    _need(260, 64)
    return _run("big_c5_check.py", "every", timeout=3000, check=False)


def test_config3_full_size_against_the_oracle(config3_run):
    lines = _part(config3_run, "sampled walkers", "config 3 at full size:")
    assert sum("IDENTICAL" in ln for ln in lines) >= 3


def test_config5_stand_in_full_size_against_the_oracle(config5_run):
    lines = _part(config5_run, "sampled walkers", "config 5 stand-in at full size:")
    assert sum("IDENTICAL" in ln for ln in lines) >= 1


def test_config3_every_walker_through_independent_samplers(config3_run):
    """One iteration at walkLength 80: the default table path, the other table kernel and the on-the-fly samplers (tables off) agree on ALL
    8.9 M walkers; boundary draws (the tie list, the chain kernels, hand-overs) are among them."""
    lines = _part(config3_run, "every walker (", "every walker at full size (c3):")
    assert sum("IDENTICAL" in ln for ln in lines) >= 3


def test_config5_stand_in_every_walker_through_independent_samplers(config5_run):
    lines = _part(config5_run, "every walker (", "every walker at full size (c5):")
    assert sum("IDENTICAL" in ln for ln in lines) >= 3


def test_config4_full_size_eight_virtual_shards_and_the_oracle():
    _need(240, 64)
    _, out = _run("big_c4_check.py", "27", "8")
    assert out.count("IDENTICAL") >= 2 and "oracle:" in out


def test_sharded_tables_at_config3_size():
    _need(250, 24)
    _, out = _run("big_shard_tables_check.py", "24", "16", "1", "0", "0.25", "4", "1", "2")
    assert out.count("IDENTICAL") >= 2          # world 1 with one walker population, world 2 with two
