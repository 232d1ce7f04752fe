"""The owner types of ``artalk_amd/csrc/device_mem.h`` (DevBuf, PinnedBuf, Event, StageTimer) under the address and undefined-behaviour
sanitizers, on the host: ``tools/host_check/device_mem_check.cpp`` is built into a temporary directory and run as a child process that
sees no device, so every HIP call it makes fails and every method takes its failure path - alloc, grow, upload, reset, move-construct,
move-assign, double reset, a timer abandoned without ``finish`` and a disabled timer.  The program checks after each failure that the
object is empty with capacity 0 and that no error is left behind; here: exit status 0 and not a word from a sanitizer."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owner_types_run_clean_under_the_sanitizers(tmp_path):
    src = os.path.join(REPO, "tools", "host_check")
    made = subprocess.run(["make", "-C", src, f"OUT={tmp_path}"], capture_output=True, text=True)
    assert made.returncode == 0, made.stdout + made.stderr
    flags = open(os.path.join(src, "Makefile")).read()
    assert "-Xarch_host -fsanitize=address,undefined" in flags
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="")      # the failure paths, on every machine
    run = subprocess.run([str(tmp_path / "device_mem_check")], capture_output=True, text=True, env=env)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stderr == "", run.stderr
    assert "checks held (no device: failure paths)" in run.stdout
