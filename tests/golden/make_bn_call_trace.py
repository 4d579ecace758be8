"""Records the library calls of the batch-norm ops: every case of tests/test_bn_calls.py, run as that test runs it (CPU tensors, a
recording stand-in for the library; needs the built libvnet_hip.so, no GPU).

    python tests/golden/make_bn_call_trace.py

Output: tests/golden/bn_call_trace.json, {case: {"calls": [[entry point, [arguments]], ...], "out": ..., "grads": ...}}.  The file
pins what the ops did BEFORE bn_act, bn_chain and bn_head were put behind one autograd function: it was written from the commit in
front of that change and is not to be regenerated to make a changed op pass -- a launch, an argument or an order that moves is a
change of the step, to be made on purpose and shown in the diff of the JSON."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import test_bn_calls as T  # noqa: E402


def main():
    traces = dict((name, T.CASES[name]()) for name in sorted(T.CASES))
    with open(T.GOLDEN, "w") as f:
        json.dump(traces, f, indent=0, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print("%d cases, %d calls -> %s" % (len(traces), sum(len(t["calls"]) for t in traces.values()), T.GOLDEN))


if __name__ == "__main__":
    main()
