"""The weight intake of ``artalk_amd/csrc/weight_store.h`` (WeightStore, pack_conv_weight) and the CallTimer and WsLayout of
``device_mem.h`` under the address and undefined-behaviour sanitizers, on the host: ``tools/host_check/weight_store_check.cpp`` is built
into a temporary directory and run as a child process that sees no device.  The program checks the declaration order, torch's wording
for an unknown key, a wrong rank and a wrong extent, that a key set twice keeps the later data, the missing-key report at 8 and at 9
names and with an optional key, the conv repack against a plain triple loop with padded rows, and - every HIP call failing - that
``upload`` and the timer fail quietly; here: exit status 0 and not a word from a sanitizer."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_weight_intake_and_call_timer_run_clean_under_the_sanitizers(tmp_path):
    src = os.path.join(REPO, "tools", "host_check")
    made = subprocess.run(["make", "-C", src, f"OUT={tmp_path}", f"{tmp_path}/weight_store_check"], capture_output=True, text=True)
    assert made.returncode == 0, made.stdout + made.stderr
    flags = open(os.path.join(src, "Makefile")).read()
    assert "-Xarch_host -fsanitize=address,undefined" in flags
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="")      # the failure paths, on every machine
    run = subprocess.run([str(tmp_path / "weight_store_check")], capture_output=True, text=True, env=env)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stderr == "", run.stderr
    assert "checks held (no device: failure paths)" in run.stdout
