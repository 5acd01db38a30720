"""Walks from a caller-supplied list of start vertices — what can be checked without a GPU: the new symbols, the parse rules of
the --sources file (srw_parse_sources: the id rule of an edge list's columns), the CLI's option handling.
The walks themselves: tests/test_gpu_sources.py."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

from conftest import KARATE
from helpers import pkg

NO_GPU = not torch.cuda.is_available()


def _cli(*args):
    return subprocess.run([pkg().CLI_PATH, *args], capture_output=True, text=True, timeout=120)


def test_new_symbols_are_exported_and_refuse_a_null_handle():
    P = pkg()
    L = P.lib()
    for sym in ("srw_set_sources", "srw_set_sources_device", "srw_clear_sources", "srw_sources", "srw_parse_sources"):
        assert sym in P.EXPORTS and hasattr(L, sym), sym
    ids = np.array([1, 2, 3], dtype=np.int32)
    n = C.c_int64(7)
    assert L.srw_set_sources(None, ids.ctypes.data_as(C.POINTER(C.c_int32)), 3) == P.ERR_INVALID
    assert L.srw_set_sources_device(None, None, 0) == P.ERR_INVALID
    assert L.srw_clear_sources(None) == P.ERR_INVALID
    assert L.srw_sources(None, C.byref(n)) == P.ERR_INVALID
    for name in ("set_sources", "clear_sources", "sources_len"):
        assert callable(getattr(P.Engine, name))


def test_parse_sources_reads_ids_by_the_edge_list_rule(tmp_path):
    P = pkg()
    f = tmp_path / "s.txt"
    f.write_bytes("3 1\t1\n\n  -2147483648\r\n2147483647 \x0b+7\x0c１２ ٣\n0".encode("utf-8"))
    got = P.parse_sources(str(f))
    assert got.dtype == np.int32
    assert got.tolist() == [3, 1, 1, -2147483648, 2147483647, 7, 12, 3, 0]       # file order, duplicates kept, fullwidth / Arabic-Indic digits
    f.write_bytes(b"")
    assert P.parse_sources(str(f)).tolist() == []                                # an empty file: an empty list
    f.write_bytes(b" \n\t\r\n")
    assert P.parse_sources(str(f)).tolist() == []
    f.write_bytes(b"\xef\xbb\xbf5 6\n")                                          # a byte order mark, as for an edge list
    assert P.parse_sources(str(f)).tolist() == [5, 6]


@pytest.mark.parametrize("text,line,token", [("1 2\n3 x4\n", 2, "x4"), ("1\n2\n2147483648\n", 3, "2147483648"), ("-2147483649", 1, "-2147483649"),
                                              ("1.0", 1, "1.0"), ("7 -\n", 1, "-"), ("1\r2\r\n0x10", 3, "0x10")])
def test_parse_sources_rejects_what_parseInt_rejects(tmp_path, text, line, token):
    P = pkg()
    f = tmp_path / "bad.txt"
    f.write_text(text)
    with pytest.raises(P.SrwError) as ei:
        P.parse_sources(str(f))
    assert ei.value.code == P.ERR_PARSE
    msg = str(ei.value)
    assert "NumberFormatException" in msg and ("line %d:" % line) in msg and ('"%s"' % token) in msg, msg


def test_parse_sources_missing_file(tmp_path):
    P = pkg()
    with pytest.raises(P.SrwError) as ei:
        P.parse_sources(str(tmp_path / "nope.txt"))
    assert ei.value.code == P.ERR_IO and "Input path does not exist" in str(ei.value)


def test_cli_sources_option(tmp_path):
    usage = _cli("--help").stdout
    assert "--sources <value>" in usage
    f = tmp_path / "src.txt"
    f.write_text("1 34\n2\n")
    base = ("--cmd", "randomwalk", "--input", KARATE, "--output", str(tmp_path / "out"))
    r = _cli(*base, "--sources", "/nonexistent/sources.txt")
    assert r.returncode == 1 and "Input path does not exist" in r.stderr
    assert not (tmp_path / "out").exists()
    bad = tmp_path / "bad.txt"
    bad.write_text("1\ntwo\n")
    r = _cli(*base, "--sources", str(bad))
    assert r.returncode == 1 and "NumberFormatException" in r.stderr and "line 2" in r.stderr and '"two"' in r.stderr
    r = _cli(*base, "--sources", str(f), "--gpus", "2")                        # refused by the parser: the usage text follows the error
    assert r.returncode == 1 and "--sources needs --gpus 1" in r.stderr and "Usage:" in r.stderr
    r = _cli("--cmd", "embedding", "--input", KARATE, "--output", str(tmp_path / "out"), "--sources", str(f))
    assert r.returncode == 1 and "--sources applies to" in r.stderr
    r = _cli(*base, "--sources")
    assert r.returncode == 1 and "Missing value after --sources" in r.stderr


@pytest.mark.skipif(not NO_GPU, reason="box has a GPU; the --sources run itself is in test_gpu_sources.py")
def test_cli_sources_without_a_gpu_fails_loudly(tmp_path):
    f = tmp_path / "src.txt"
    f.write_text("1 34\n2\n")
    for cmd in ("randomwalk", "node2vec"):
        r = _cli("--cmd", cmd, "--input", KARATE, "--output", str(tmp_path / "out"), "--sources", str(f))
        assert r.returncode == 1 and "no usable HIP device" in r.stderr          # never a CPU path
        assert not (tmp_path / "out").exists()
