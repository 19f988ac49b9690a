"""CPU: the flat kernel's per-descriptor image (dynamicgo_amd/csrc/
flat_image.h), built by the library's own builder in a stand-alone program
(flat_image_host.cpp) under the address and undefined-behaviour sanitizers:
the Simple blob, blobs whose lengths are and are not multiples of 16, and the
largest blob the flat kernel takes. Lengths, padding and the three tables
against P10, the powers of ten and the DG_POW10_M128 window."""
import os
import subprocess

import pytest

import descgen
from dynamicgo_amd import build as B
from dynamicgo_amd import thrift as T, workloads as W

HERE = os.path.dirname(os.path.abspath(__file__))
TABS = 864  # 8 * (20 + 23 + 64), padded to 16


def test_image_builder_under_sanitizers(tmp_path):
    if not os.path.exists(B.HIPCC):
        pytest.skip("no %s to build the host program with" % B.HIPCC)
    exe = str(tmp_path / "flat_image")
    subprocess.run([B.HIPCC, "-x", "hip", "--offload-arch=" + B.ARCH, "-O1", "-std=c++17", "-fPIC", "-ffp-contract=off",
                    "-Wno-ignored-attributes", "-Xarch_host", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(HERE, "flat_image_host.cpp")], check=True)
    blobs = [T.flatten(W.simple_desc()).blob, T.flatten(W.mixed_desc()).blob,
             T.flatten(descgen.sized_desc(6144 + 8)).blob, T.flatten(descgen.sized_desc(16384)).blob]
    assert len(blobs[0]) % 16 == 8 and len(blobs[2]) % 16 == 8 and len(blobs[3]) % 16 == 0
    files = []
    for k, b in enumerate(blobs):
        files.append(str(tmp_path / ("blob%d.bin" % k)))
        with open(files[-1], "wb") as fh:
            fh.write(b)
    out = subprocess.run([exe] + files, check=True, capture_output=True, text=True).stdout.splitlines()
    assert out == ["blob %d: image %d bytes, tables at %d: ok" % (len(b), (len(b) + 15) // 16 * 16 + TABS, (len(b) + 15) // 16 * 16)
                   for b in blobs], out
    # a damaged file is told apart: the program does not pass whatever it is given
    assert subprocess.run([exe, str(tmp_path / "missing.bin")], capture_output=True).returncode != 0
