"""The RT Dose switches of examples/raytracedicom_main.cpp end to end on the 64^3 water cube of the other CLI tests: --rtdose writes
dose.dcm (quantised on the device), --reference_rtdose reads such a file, uploads its integers, resamples them onto the dose grid and
prints the gamma line. The files are checked with the Python reader of tests/rtdose_fixture.py, which shares no code with the C++ side."""
import re
import subprocess

import numpy as np
import pytest

import rtdose_fixture as fx
import rtdose_support
from raytracedicom_amd import luts

pytestmark = pytest.mark.gpu

N = 64
GAMMA_LINE = re.compile(r"^gamma\(([0-9.]+)%/([0-9.]+)mm\): ([0-9.]+) % of ([0-9]+) voxels, max ([0-9.]+)$", re.M)


@pytest.fixture(scope="module")
def cli(tmp_path_factory, synth):
    """The built example, a LUT directory and the first run: --rtdose --rtdose_bits 32."""
    tmp = tmp_path_factory.mktemp("rtdose_cli")
    exe = rtdose_support.build_cli(tmp)
    lut_dir = str(tmp / "luts")
    luts.write_lut_dir(lut_dir, synth)
    out = tmp / "out"
    out.mkdir()
    base = [exe, "--water_cube", "--water_cube_edge", str(N), "--layers", "2", "--lut_dir", lut_dir, "--gpu_id", "0"]
    r = subprocess.run(base + ["--output_directory", str(out), "--rtdose", "--rtdose_bits", "32"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return dict(base=base, tmp=tmp, out=out, first=r)


def run(cli, name, *extra):
    out = cli["tmp"] / name
    out.mkdir()
    r = subprocess.run(cli["base"] + ["--output_directory", str(out)] + list(extra), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r, out


def test_rtdose_is_the_dose_on_the_ct_grid(cli):
    dose = np.fromfile(str(cli["out"] / "dose.dat"), dtype=np.float32).reshape(N, N, N)
    got = fx.read_rtdose(str(cli["out"] / "dose.dcm"))
    s = got["scaling"]
    assert got["dims"] == (N, N, N) and got["pixels"].dtype == np.uint32 and dose.max() > 0
    err = np.abs(got["dose"] - dose.astype(np.float64)).max()
    print("DoseGridScaling %s, largest error %.6g steps" % (got["scaling_text"], err / s))
    assert err <= s / 2 * (1 + 2.0 ** -20)
    assert int(got["pixels"].max()) >= 2 ** 32 - 8                    # the scale was chosen from the largest dose
    voxel = 256.0 / N                                                 # the water cube's grid: main.cu:43
    assert np.allclose(got["matrix"], np.diag([voxel] * 3), rtol=1e-9) and np.allclose(got["origin"], (-128.0, -128.0, -106.0), rtol=1e-9)
    assert got["offsets"][0] == 0.0 and got["units"] == "GY" and got["dose_type"] == "PHYSICAL"
    assert "Written " + str(cli["out"]) + "/dose.dcm (32 bits" in cli["first"].stdout and "rtdose=true" in cli["first"].stdout


def test_without_the_switches_nothing_is_added(cli):
    r, out = run(cli, "plain")
    assert not (out / "dose.dcm").exists() and "rtdose=" not in r.stdout and "dose.dcm" not in r.stdout and "gamma" not in r.stdout
    assert (out / "dose.dat").read_bytes() == (cli["out"] / "dose.dat").read_bytes()


def test_reference_on_the_same_grid_passes_everywhere(cli):
    r, out = run(cli, "same", "--reference_rtdose", str(cli["out"] / "dose.dcm"), "--gamma", "1,1")
    m = GAMMA_LINE.search(r.stdout)
    assert m, r.stdout[-600:]
    assert (float(m.group(1)), float(m.group(2))) == (1.0, 1.0) and float(m.group(3)) == 100.0 and int(m.group(4)) > 0


def test_reference_on_a_coarser_descending_grid(cli):
    """Reader -> integer upload -> resample -> gamma. The reference is every second voxel of the written dose, its frames stacked
    downwards. There is no bar on the rate: nobody has measured what 8 mm sampling of this field gives."""
    src = fx.read_rtdose(str(cli["out"] / "dose.dcm"))
    coarse = np.ascontiguousarray(src["pixels"][::2, ::2, ::2][::-1])
    voxel = 256.0 / N
    top = -106.0 + voxel * 2 * (coarse.shape[0] - 1)                  # frame 0 of the rewritten file is the highest slice
    path = str(cli["tmp"] / "coarse.dcm")
    fx.write_rtdose(path, coarse, src["scaling"], scaling_text=src["scaling_text"], origin=(-128.0, -128.0, top), spacing=(2 * voxel,) * 3,
                    descending=True, syntax=fx.IMPLICIT)
    r, out = run(cli, "coarse", "--reference_rtdose", path, "--gamma", "3,3")
    m = GAMMA_LINE.search(r.stdout)
    assert m, r.stdout[-600:]
    print(m.group(0))
    assert (float(m.group(1)), float(m.group(2))) == (3.0, 3.0) and int(m.group(4)) > 0
    assert 0.0 <= float(m.group(3)) <= 100.0 and np.isfinite(float(m.group(5)))
