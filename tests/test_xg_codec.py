"""The tagged-granule record codecs (ops/csrc/xg_codec.h) on the CPU: the
stand-alone program tests/xg_codec_check.cpp is compiled as plain host C++
(address and undefined-behaviour sanitizers on where the compiler links them)
and run."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "sharding-the-sphere-fall-2025-jax-devlab-examples_amd", "ops", "csrc")


def _compilers():
    for c in (os.environ.get("CXX"), "g++", "clang++"):
        p = shutil.which(c) if c else None
        if p:
            yield [p]
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            yield [c, "-x", "c++"]


def test_xg_codecs_roundtrip_bit_for_bit(tmp_path):
    exe = str(tmp_path / "xg_codec_check")
    src = os.path.join(HERE, "xg_codec_check.cpp")
    errors = []
    for cc in _compilers():
        # (the address sanitizer linked statically: its shared runtime refuses
        # to start behind any other preloaded library)
        for san in (["-fsanitize=address,undefined", "-static-libasan"], ["-fsanitize=undefined"], None):
            san = [*san, "-fno-sanitize-recover=all"] if san else []
            cmd = [*cc, "-std=c++17", "-O1", "-g", *san, "-I", CSRC, src, "-o", exe]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode == 0:
                break
            errors.append(" ".join(cmd) + "\n" + r.stdout + r.stderr)
        else:
            continue
        break
    else:
        if not errors:
            pytest.skip("no host C++ compiler found")
        pytest.fail("xg_codec_check.cpp did not compile:\n" + "\n".join(errors))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "xg codecs ok" in r.stdout
