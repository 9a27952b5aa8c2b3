#!/usr/bin/env python
"""Generate tests/golden/launch_traces.json: per configuration of tests/launch_trace.py the number of libmmrca calls of one
forward (+ backward) and, per call, the entry point and a short digest of its canonical line.

    python tests/golden/make_launch_traces.py [--dump DIR] [--out FILE]

Needs neither a GPU nor libmmrca.so.  The committed file records the launch sequences of the engines BEFORE the per-layer forwards
of engine.py and q_former.py were folded into one function each; it is the fixed point host-side refactors are held to and is not
regenerated when engine code changes (a pull request that changes a launch on purpose regenerates it and shows the diff of two
--dump directories).  To repeat the recording: check out garbage_classification_rca_amd/ as of the commit before this file was added,
run this script, and compare the JSON byte for byte.

--dump DIR also writes the full canonical text, one file per configuration, so that two versions of the engines can be diffed.
"""
import argparse
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from tests import launch_trace as LT  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "launch_traces.json"))
    ap.add_argument("--dump", default=None, metavar="DIR")
    args = ap.parse_args()
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
    out = {}
    for name in LT.CONFIGS:
        with pytest.MonkeyPatch.context() as mp:
            lines = LT.trace(name, mp)
        out[name] = {"count": len(lines), "calls": [LT.entry(ln) for ln in lines]}
        if args.dump:
            with open(os.path.join(args.dump, name + ".txt"), "w") as f:
                f.write("\n".join(lines) + "\n")
        print(f"{name}: {len(lines)} calls")
    with open(args.out, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in out.items()) + "\n}\n")
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
