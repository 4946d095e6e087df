"""Build helpers shared by the RT Dose tests: the stand-alone C++ driver of the reader and writer, and the command-line example.
A plain module (no tests)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_SRC = os.path.join(ROOT, "tests", "cpp", "test_rtd_rtdose.cpp")


def build_driver(tmp_path, sanitize=False):
    exe = str(tmp_path / ("test_rtd_rtdose_san" if sanitize else "test_rtd_rtdose"))
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")] + extra + [DRIVER_SRC, "-o", exe])
    return exe


def build_cli(tmp_path):
    from raytracedicom_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        engine.build()
    exe = str(tmp_path / "raytracedicom")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "examples"),
                           os.path.join(ROOT, "examples", "raytracedicom_main.cpp"), "-L", os.path.join(ROOT, "raytracedicom_amd"),
                           "-lrtd_hip", "-Wl,-rpath," + os.path.join(ROOT, "raytracedicom_amd"), "-o", exe])
    return exe
