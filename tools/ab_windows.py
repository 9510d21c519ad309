"""Run one of tools/bench_*.py from a given tree and keep every timing window it takes, not only the median it prints.

    python tools/ab_windows.py TREE TOOL LOG.json REPS -- [the tool's own arguments]

TREE is the checkout to measure (this one, or a built worktree of the commit to compare with: run them in turn, in one
session); REPS is how often the tool's main() runs in the process.  profiles/raycast_refactor.txt was recorded this way.
The tool runs as it is (its main()); window_ms / timed are wrapped so that each window's ms per call is recorded under
the source line of the callable it timed (the tools are the same files in both trees, so the lines name the variants).
"""
import importlib
import json
import os
import sys

tree, tool, log, reps = os.path.abspath(sys.argv[1]), sys.argv[2], os.path.abspath(sys.argv[3]), int(sys.argv[4])
rest = sys.argv[sys.argv.index("--") + 1:]
os.chdir(tree)
sys.path[:0] = [os.path.join(tree, "tools"), tree]

records = []


def wrap(orig):
    if getattr(orig, "_wrapped", False):
        return orig

    def w(fn, *a, **k):
        ms = orig(fn, *a, **k)
        records.append(["%s:%d" % (os.path.basename(fn.__code__.co_filename), fn.__code__.co_firstlineno), ms])
        return ms
    w._wrapped = True
    return w


import bench_map  # noqa: E402
import tools.bench_map as tbm  # noqa: E402

bench_map.window_ms = wrap(bench_map.window_ms)
tbm.window_ms = wrap(tbm.window_ms)
mod = importlib.import_module(tool)
for name in ("window_ms", "timed"):
    if name in mod.__dict__:
        setattr(mod, name, wrap(mod.__dict__[name]))

import occdepth_amd  # noqa: E402
assert os.path.abspath(occdepth_amd.__file__).startswith(tree + os.sep), occdepth_amd.__file__
sys.argv = [tool] + rest
for _ in range(reps):
    mod.main()
by = {}
for key, ms in records:
    by.setdefault(key, []).append(round(ms, 5))
with open(log, "w") as f:
    json.dump({"tree": tree, "tool": tool, "windows": by}, f, indent=1)
print("AB", tool, tree, json.dumps(by))
