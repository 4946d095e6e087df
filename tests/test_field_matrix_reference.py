"""The life of a field's dose-influence matrix (raytracedicom_amd/csrc/rtd_field_matrix.hpp: what exists of it, what it is valid for,
the element counts of the buffer table) against the loose members and the assignments the engine once wrote out by hand, transcribed
in tests/cpp/test_rtd_field_matrix.cpp: a stand-alone program that walks both in lock step over random event sequences (fixed seed)
and compares every observable after every event, run plain and under the address and undefined-behaviour sanitizers (no GPU needed)."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "test_rtd_field_matrix.cpp")
CSRC = os.path.join(ROOT, "raytracedicom_amd", "csrc")


def build(tmp_path, sanitize):
    exe = str(tmp_path / ("test_rtd_field_matrix_san" if sanitize else "test_rtd_field_matrix"))
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC] + extra + [SRC, "-o", exe])
    return exe


@pytest.mark.parametrize("sanitize", (False, True), ids=("plain", "sanitizers"))
def test_matrix_record_equals_the_hand_written_members(tmp_path, sanitize):
    """4000 walks x 64 events. The driver has its own main and refuses (exit code 3) a walk on which some observable keeps one value or
    a named sequence (prepared, LET values valid, then the matrix computed again; a failed computation over a listed companion; ...) is
    never reached; with -fsanitize=address,undefined a finding aborts it."""
    r = subprocess.run([build(tmp_path, sanitize)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 2 and lines[0].startswith("transcription ") and lines[1].startswith("ok ")
    assert lines[0].split()[1:] == lines[1].split()[1:]                 # the lock step walked the events the transcription alone did
    n = [int(x) for x in re.findall(r"\d+", lines[1])]
    assert n[0] == 4000 * 64 and min(n) > 0                             # every value of every observable was taken


def test_the_header_is_host_only():
    """Plain C++ that compiles alone (the build above), and nothing of HIP or of the kernels' headers in it."""
    text = open(os.path.join(CSRC, "rtd_field_matrix.hpp")).read()
    includes = re.findall(r"#include\s*[<\"]([^>\"]+)[>\"]", text)
    assert includes and all(not i.startswith("hip") and not i.startswith("rtd_") for i in includes), includes
