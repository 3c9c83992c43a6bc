"""CPU: AddressSanitizer + UndefinedBehaviorSanitizer over the host (emulator) build of csrc/geom_verify.hip, as a stand-alone program with
its own main (tests/sanitize/gv_sanitize_main.cpp): nk = 8193 (streaming kernels, both chunk layouts) and nk = 100 (LDS-resident kernels)."""
import importlib
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_streaming_verification_is_clean_under_asan_and_ubsan(tmp_path):
    build = importlib.import_module("deep-image-matching_amd.build")
    emu = ROOT / "tests" / "hipemu"
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fPIC", "-ffp-contract=off", "-Wno-psabi", "-Wno-unused-value",
             "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", str(emu / "include"), "-I", str(ROOT / "include")]
    exe = tmp_path / "gv_sanitize"
    srcs = [ROOT / "tests" / "sanitize" / "gv_sanitize_main.cpp", build.CSRC / "geom_verify.hip", emu / "hipemu.cpp"]
    cmd = [build.HOST_CLANG, *flags, "-o", str(exe)]
    for s in srcs:
        cmd += ["-x", "c++", str(s)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
