"""The dose record's part of what a field keeps between computes (raytracedicom_amd/csrc/rtd_field_memory.hpp): it is allocated,
recorded, usable and dropped with the sigma record, changes nothing about the sigma record's own decisions, and a failure of its
allocation alone leaves the field replaying sigma. tests/cpp/test_rtd_dose_record.cpp is a stand-alone program that walks the header
over random event sequences (fixed seed) and checks these rules after every event, run plain and under the address and
undefined-behaviour sanitizers (no GPU needed)."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "test_rtd_dose_record.cpp")
CSRC = os.path.join(ROOT, "raytracedicom_amd", "csrc")


@pytest.mark.parametrize("sanitize", (False, True), ids=("plain", "sanitizers"))
def test_dose_record_follows_the_sigma_record(tmp_path, sanitize):
    """8 configurations x 1500 walks x 96 events. The driver has its own main and refuses (exit code 3) a walk on which some observable
    keeps one value; with -fsanitize=address,undefined a finding aborts it."""
    exe = str(tmp_path / ("test_rtd_dose_record_san" if sanitize else "test_rtd_dose_record"))
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC] + extra + [SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("ok ")
    n = [int(x) for x in re.findall(r"\d+", lines[0])]
    assert n[0] == 8 * 1500 * 96 and min(n) > 0                         # every value of every observable was taken
