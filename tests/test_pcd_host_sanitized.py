"""The host half of the PCD codec (fastdem_amd/csrc/fdm_pcd_host.hpp) under AddressSanitizer and
UndefinedBehaviorSanitizer, as a stand-alone program: fastdem_amd/cpp/tests/pcd_host_probe.cpp is compiled here with
g++ -fsanitize=address,undefined and run over the header cases, the truncation sweep and the ASCII files of the other
PCD tests.  Every input is copied into a heap block of exactly its size, so a read behind `n_bytes` is a report; what
the program prints is held to the restatement (tests/pcd_restate.py).  Nothing sanitized is loaded into Python."""
import os
import subprocess

import pytest

import pcd_cases as PC
import pcd_restate as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "fastdem_amd", "cpp", "tests", "pcd_host_probe.cpp")
SWEEPS = ["valid", "crlf", "pcl_xyzrgbnormal", "viewpoint_eight_numbers", "fields_65"]


SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pcd_probe")
    # can this toolchain link and run the sanitizers at all?  Asked with a trivial program, so that whatever goes wrong
    # with the real one afterwards is a failure, not a skip
    trivial = tmp / "trivial.cpp"
    trivial.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++", *SANITIZE, str(trivial), "-o", str(tmp / "trivial")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp / "trivial")], capture_output=True).returncode != 0:
        pytest.skip("this toolchain cannot link the sanitizers: " + r.stderr[-300:])
    out = str(tmp / "pcd_host_probe_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fno-omit-frame-pointer", *SANITIZE, SRC, "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def run(probe, args):
    r = subprocess.run([probe] + args, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-4000:]
    assert b"runtime error" not in r.stderr and b"Sanitizer" not in r.stderr, r.stderr.decode(errors="replace")[-4000:]
    sections, cur = [], None
    for line in r.stdout.decode("latin-1").split("\n"):
        if line.startswith("== "):
            cur = []
            sections.append(cur)
        elif cur is not None:
            cur.append(line)
    return [s[:-1] if s and s[-1] == "" else s for s in sections]


def test_header_cases_and_truncation_sweep(probe, tmp_path):
    args, want = [], []
    for name in sorted(PC.HEADERS):
        path = str(tmp_path / (name + ".pcd"))
        with open(path, "wb") as f:
            f.write(PC.HEADERS[name])
        args += ["header", path]
        want.append([PC.digest(PC.restated(PC.HEADERS[name]))])
    for name in SWEEPS:
        data = PC.HEADERS[name]
        args += ["sweep", str(tmp_path / (name + ".pcd"))]
        want.append([PC.digest(PC.restated(data[:cut])) for cut in range(len(data) + 1)])
    got = run(probe, args)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, args[2 * k + 1]


def test_ascii_codec(probe, tmp_path):
    from test_pcd_ascii import DECODE_FILES
    files = dict(DECODE_FILES)
    valid = DECODE_FILES["all_channels"]
    for cut in range(len(valid) - 60, len(valid) + 1):                    # records cut short at every byte of the tail
        files[f"cut_{cut}"] = valid[:cut]
    args, want = [], []
    for name in sorted(files):
        path = str(tmp_path / (name + ".pcd"))
        with open(path, "wb") as f:
            f.write(files[name])
        args += ["ascii", path]
        try:
            h, c = PR.load(files[name])
            if h.format != PR.ASCII:
                raise PR.PcdError("not ascii")
            text = ""
            for precision in (8, 3):
                text += f"precision {precision}\n" + PR.save_body(c, PR.ASCII, precision).decode()
            want.append(text.split("\n")[:-1])
        except PR.PcdError:
            want.append(["error"])
    got = run(probe, args)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, args[2 * k + 1]
