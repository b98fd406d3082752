"""The toolkit of the CPU harnesses under tests/host/: each compiles one host/device header of the product with plain g++ and
runs it on lines read from stdin, one line group per problem, one or more output lines per problem.  Here: the build (one set
of flags), the number formatting, the run with its checks, the fixture loader, and the comparisons and the row count that
several families' tests share.  The *_util.py modules keep what is their
family's own: the line grammar and the numpy / torch restatements."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def build(source_name, tmp_path, sanitize=False):
    """tests/host/<source_name> -> executable under tmp_path.  Contraction off, as in the product's headers: the harness and the
    kernel execute the same operations.  sanitize: AddressSanitizer + UndefinedBehaviorSanitizer, no recovery."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler for tests/host/" + source_name)
    stem = os.path.splitext(source_name)[0]
    exe = str(tmp_path / (stem + "_san" if sanitize else stem))
    flags = ["-std=c++17", "-ffp-contract=off"]
    flags += ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run([cxx] + flags + [os.path.join(ROOT, "tests", "host", source_name), "-o", exe], check=True, capture_output=True,
                   text=True)
    return exe


def fmt(a):
    """the doubles of an array, each as the shortest text that reads back to the same bits"""
    return " ".join(repr(float(x)) for x in np.asarray(a, dtype=np.float64).reshape(-1))


def ints(a):
    """the integers of an array as text"""
    return " ".join(str(int(x)) for x in np.asarray(a).reshape(-1))


def run(exe, lines, expected, timeout=600, env=None):
    """feeds the joined lines to the harness -> its `expected` output lines, raw (exit code 0 and the line count asserted)"""
    r = subprocess.run([exe], input="".join(lines), capture_output=True, text=True, timeout=timeout,
                       env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    out = r.stdout.strip("\n").split("\n") if expected else []
    assert len(out) == expected, (len(out), r.stderr[-2000:])
    return out


def load_cases(fixture_name):
    """the "cases" of tests/golden/<fixture_name>"""
    with open(os.path.join(GOLDEN, fixture_name)) as f:
        return json.load(f)["cases"]


def live_rows(n_samples, status, capacity):
    """the rows a plan step sees of a path: none of a path with status <= 0, else its count held to [0, capacity]"""
    return 0 if status <= 0 else max(min(int(n_samples), int(capacity)), 0)


def same_bits(a, b):
    """bit for bit, a NaN equal to any NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    return bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))


def grads_agree(got, want, scale, rtol):
    """|got - want| <= rtol * scale entry by entry (no NaN on either side)"""
    got, want = np.asarray(got), np.asarray(want)
    return bool(np.all(np.isfinite(got)) and np.all(np.abs(got - want) <= rtol * scale))
