"""csrc/field_state.h on the CPU: which events leave the predicate standing that lets a render read the component cache
(RecordStamps::comps_of_records, k_comps.h).  tests/host/comp_cache_stamps.cpp fires every event of FieldState and of SourceStamps
once; built as a stand-alone program with the host compiler under the address and undefined-behaviour sanitizers, like
tests/host/prep_skip_stamps.cpp.  No GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_events_keep_or_drop_the_component_cache_predicate(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "comp_cache_stamps")
    # (the sanitizers' runtimes linked INTO the program -- clang's default)
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static +
                   ["-I", os.path.join(ROOT, "desi-mcmc_amd", "csrc"), os.path.join(ROOT, "tests", "host", "comp_cache_stamps.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "comp_cache_stamps: ok", run.stdout + run.stderr
