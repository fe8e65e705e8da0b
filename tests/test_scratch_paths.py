"""The failure paths of the host code's scratch, buffer and timer types (pyfocusr_amd/csrc/pf_scratch.h) on the CPU: the header
over test doubles of the device allocator and of the event calls that fail on the n-th call, built with the address and undefined-behaviour
sanitizers and run as a program of its own (tests/csrc/scratch_paths.cpp says what it checks).  No GPU, no HIP runtime."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "scratch_paths.cpp")
HDR = os.path.join(HERE, "..", "pyfocusr_amd", "csrc", "pf_scratch.h")
EXE = os.path.join(HERE, "_build", "scratch_paths")
# the HIP headers (types and prototypes only) lie beside the compiler the library is built with
HIP_INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))), "include")


def build():
    if not os.path.exists(EXE) or any(os.path.getmtime(p) > os.path.getmtime(EXE) for p in (SRC, HDR)):
        os.makedirs(os.path.dirname(EXE), exist_ok=True)
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-D__HIP_PLATFORM_AMD__", "-I", HIP_INCLUDE, "-o", EXE, SRC], check=True)
    return EXE


def test_scratch_and_devbuf_failure_paths_under_sanitizers():
    run = subprocess.run([build()], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert run.returncode == 0, run.stdout
    assert run.stdout.strip().splitlines()[-1] == "ok", run.stdout
