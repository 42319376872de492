#!/usr/bin/env python3
"""Generates tests/golden/reference_digests.npz from the REAL reference: what it returned for the inputs of the tests that compare with it
(helpers.StoredReference), so that those comparisons also run where the reference cannot be built.

Build container only: needs oracle/_ref/libstbref.so (the reference compiled in place by oracle/Makefile).  It runs those tests with
REF_DIGESTS_RECORD set, so every answer is recorded for exactly the input a test declares.  Everything stored is DATA, one entry per
call, keyed by the SHA-256 of the call and its input:
  load/<req>/<pixels>   "fail:<reason>", or "ok:<shape>:<comp>:<SHA-256 of the pixels>" ("ok" alone where pixels are not compared)
  encode/<shape>/<q>    "<length>:<SHA-256>" of the writer's stream
  idct                  "<length>:<SHA-256>" of the 8x8 output block
  verdicts/<req>/<group> one entry per generated list of streams (tests/stream_cases.py), keyed over all of them: one character per
                        stream ('0' ok, '1'.. a reason) and the reasons behind it -- verdict and reason only, no pixels
  info                  "1 <x> <y> <comp>" or "0": stbi_info_from_memory

The header families (tests/header_cases.py) are recorded in a child process each: the reference is built with its assertions live and
ABORTS where a stream strays outside what it defines (a table used before it was defined, ...).  An abort here is an error of the case
generator: the case belongs into header_cases.product_only, or the generator is wrong.  Nothing is written then.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "reference_digests.npz")
TESTS = [
    "tests/test_oracle_golden.py::test_oracle_vs_live_reference_seeded",
    "tests/test_oracle_golden.py::test_oracle_vs_live_reference_fuzz",
    "tests/test_oracle_golden.py::test_oracle_vs_live_reference_sampling_layouts",
    "tests/test_host_cpu.py::test_host_writer_vs_live_reference_seeded",
    "tests/test_host_cpu.py::test_progressive_host_walk_vs_oracle_fuzz",
    "tests/test_host_cpu.py::test_third_pair_of_huffman_tables_host_walk",
    "tests/test_stream_ends_host.py::test_progressive_cuts_host_walk_vs_oracle",
    "tests/test_stream_ends_host.py::test_baseline_stream_ends_host_walk_and_extract_gate",
    "tests/test_progressive_writer.py::test_progressive_stream_carries_the_same_coefficients",
    "tests/test_progressive_writer.py::test_writer_streams_pin_the_oracle_to_the_live_reference",
]
HEADER_FAMILIES = ["reasons", "segments", "frames", "scans", "tables"]

if __name__ == "__main__":
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libstbref.so")):
        sys.exit("oracle/_ref/libstbref.so is missing: make -C oracle ref (where the reference exists)")
    tmp = OUT + ".new.npz"
    if os.path.exists(tmp):
        os.remove(tmp)
    env = dict(os.environ, REF_DIGESTS_RECORD=tmp)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider"] + TESTS, cwd=ROOT, env=env)
    if r.returncode != 0:
        sys.exit("the tests failed against the reference itself: nothing written")
    for fam in HEADER_FAMILIES:
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", "tests/test_headers_host.py::test_family_host[%s]" % fam], cwd=ROOT, env=env)
        if r.returncode < 0 or r.returncode >= 128:
            sys.exit("the reference aborted on family '%s' (exit status %d): a case outside its contract -- nothing written" % (fam, r.returncode))
        if r.returncode != 0:
            sys.exit("family '%s' failed against the reference itself: nothing written" % fam)
    os.replace(tmp, OUT)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
