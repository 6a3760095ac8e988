#!/usr/bin/env python3
"""Regenerate tests/golden/golden_xmodem_recv.npz + manifest_xmodem_recv.json from the REAL XModemTransport.receiveData() (build
container only).  TEST INFRASTRUCTURE.  oracle/refrun/strip_ts.py, unchanged, type-strips the reference into a temp dir (never into
the repo); harness.js runs the class under Node against scripted data channels and dumps raw arrays and a manifest there; this
script packs them.  Only data reaches the repo: demodulate() replies, the bytes of every modulate() call, outcomes (the files), counters.

usage: python tools/xmodem_recv_golden/make_golden.py [--ref /root/reference]
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="fsk_xmodem_recv_golden_")
    try:
        subprocess.check_call([sys.executable, os.path.join(REPO, "oracle", "refrun", "strip_ts.py"), args.ref, tmp])
        out = os.path.join(tmp, "out")
        subprocess.check_call(["node", os.path.join(HERE, "harness.js"), os.path.join(tmp, "ref_bundle.js"), out])
        with open(os.path.join(out, "manifest.json")) as fh:
            man = json.load(fh)
        arrays = {}
        for name in man.pop("arrays"):
            stem, dt = name.rsplit(".", 1)
            arrays[stem] = np.fromfile(os.path.join(out, name + ".bin"), dtype={"u1": "u1", "i4": "<i4"}[dt])
        gold = os.path.join(REPO, "tests", "golden")
        path = os.path.join(gold, "golden_xmodem_recv.npz")
        np.savez_compressed(path, **arrays)
        assert os.path.getsize(path) < 1 << 20
        with open(os.path.join(gold, "manifest_xmodem_recv.json"), "w") as fh:
            json.dump(man, fh, indent=None, separators=(",", ":"))
        print("wrote %d scenarios, %d bytes" % (len(man["cases"]), os.path.getsize(path)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
