"""The stand-alone sanitizer programs of the host restatement (tools/load_*_asan.cpp): each has its own ``main``, is
built with AddressSanitizer and UndefinedBehaviorSanitizer against cadence_amd/csrc/load_states.cpp and run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_and_run(tmp_path, name: str) -> str:
    """Build tools/<name>.cpp into ``tmp_path`` and run it: exit status 0 and no sanitizer report; its stdout."""
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", name + ".cpp"),
                    os.path.join(ROOT, "cadence_amd", "csrc", "load_states.cpp"), "-o", exe, "-lpthread"], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "no sanitizer report" in p.stdout
    return p.stdout
