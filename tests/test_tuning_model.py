"""pcc_set_tuning's table (pcc-rl_amd/csrc/pcc_sim.hip) under the address and undefined-behaviour sanitizers, without a GPU:
tests/models/tuning_model.cpp holds what every key accepted before the table replaced the switch -- the ends of its range,
just outside both, NaN -- and calls the pure part of pcc_set_tuning with it."""
import os
import shutil
import subprocess

import pcc_rl_amd
from pcc_rl_amd import build as pbuild

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "models", "tuning_model.cpp")
EXE = os.path.join(HERE, "models", "tuning_model")


def test_tuning_table_accepts_what_the_switch_accepted():
    # the host code of pcc_sim.hip, instrumented, and the program; the kernels' launch functions come from the product library
    lib = pcc_rl_amd.build_library()
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fPIC",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I", pbuild.INCLUDE, "-I", pbuild.CSRC, os.path.join(pbuild.CSRC, "pcc_sim.hip"), SRC, "-o", EXE,
                           "-L", os.path.dirname(lib), "-lpcc_sim", "-Wl,-rpath," + os.path.dirname(lib)])
    run = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert run.returncode == 0 and "every key as listed" in run.stdout, run.stdout[-4000:]
