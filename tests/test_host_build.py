"""tests/host_build.py, the helper every host build of the suite goes through: when it compiles and when it does not, on a
chain a.cpp -> b.h -> c.h in a scratch directory, and what the compiler's dependency files name in the real tree. The header two
includes down is the case a hand-kept list of a source's direct includes misses."""
import os
import subprocess
import sys
import time

import pytest

from tests import host_build


def _value(so):
    """What the library's value() returns, read in a fresh process: this one keeps the image it loaded first"""
    code = "import ctypes, sys; print(ctypes.CDLL(sys.argv[1]).value())"
    return int(subprocess.check_output([sys.executable, "-c", code, so]))


def test_compiles_exactly_when_the_output_is_stale(tmp_path):
    a, b, c, so = (str(tmp_path / n) for n in ("a.cpp", "b.h", "c.h", "liba.so"))
    clock = [time.time_ns() - 1000 * 10 ** 9]

    def stamp(path):
        """The test's own clock, a second per event, all of it in the past: nothing sleeps, nothing depends on how fast it runs"""
        clock[0] += 10 ** 9
        os.utime(path, ns=(clock[0], clock[0]))

    def write(path, text):
        open(path, "w").write(text)
        stamp(path)

    def build():
        did = host_build.compile(a, so, host_build.SIM + ["-shared"])
        if did:
            stamp(so)
        return did

    write(c, "#define VALUE 41\n")
    write(b, '#include "c.h"\n')
    write(a, '#include "b.h"\nextern "C" int value() { return VALUE; }\n')
    assert host_build.shared(a, so, host_build.SIM).value() == 41  # the first call compiles, and the library loads
    stamp(so)
    at = os.stat(so).st_mtime_ns
    assert not build() and os.stat(so).st_mtime_ns == at  # fresh: nothing runs

    write(c, "#define VALUE 42\n")  # a header two includes down
    assert build() and _value(so) == 42
    assert not build()

    os.remove(so + ".d")
    assert build() and not build()

    os.remove(c)  # a header leaves together with the include that named it; b.h keeps its time, so only the missing file counts
    at = os.stat(b).st_mtime_ns
    open(b, "w").write("#define VALUE 43\n")
    os.utime(b, ns=(at, at))
    assert build() and _value(so) == 43
    assert "c.h" not in open(so + ".d").read() and not build()

    write(a, "this does not compile\n")
    for _ in range(2):  # the second time: what the failure left behind does not pass for a fresh output
        with pytest.raises(subprocess.CalledProcessError):
            build()
        assert not os.path.exists(so)
    write(a, '#include "b.h"\nextern "C" int value() { return VALUE + 1; }\n')
    assert build() and _value(so) == 44
    assert not build()


def test_the_five_pass_mirrors_compile_in_one_translation_unit(tmp_path):
    """Each shim of tests/host_sim includes one mirror of host/; a caller includes several, and all of them include
    pass_handle.hpp, so its guard and theirs are seen only here. Each mirror twice."""
    mirrors = ("resampler", "mel_spectrogram", "kaldi_features", "feature_norm", "frame_stack")
    src = str(tmp_path / "mirrors.cpp")
    host = os.path.join(host_build.ROOT, "saprobe-alac_amd", "host")
    open(src, "w").write("".join('#include "%s.hpp"\n' % os.path.join(host, m) for m in mirrors * 2) +
                         "#include <type_traits>\n"
                         "static_assert(std::is_same_v<alac::NormStrides, alac::StackStrides>, \"one struct\");\n")
    assert host_build.compile(src, str(tmp_path / "mirrors.o"), host_build.SHIM + ["-c"])


def test_dependency_files_of_the_real_tree_name_what_the_sources_include():
    from tests import kaldifft_ref
    from tests.test_chunk_pipeline_host import build_chunk_sim
    kaldifft_ref.build_fbankfft_sim()
    deps = open(os.path.join(host_build.SIM_DIR, "libfbankfft_sim.so.d")).read()
    for h in ("alac_fbankfft.h", "alac_fbank.h", "alac_melfft.h", "alac_mel.h", "alac_waveform.h"):
        assert "saprobe-alac_amd/csrc/" + h in deps, h
    build_chunk_sim()
    deps = open(os.path.join(host_build.SIM_DIR, "libchunk_sim.so.d")).read()
    assert "tests/host_sim/lane_sim.cpp" in deps and "include/alacgpu.h" in deps
    assert not any(os.path.isabs(p) for p in deps.partition(":")[2].replace("\\\n", " ").split())  # root-relative: valid wherever the tree goes
