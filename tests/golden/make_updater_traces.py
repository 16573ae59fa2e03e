"""Records tests/golden/updater_traces.json: what tests/updater_trace.py's scenarios see and
get from the FleetUpdater of a reference tree -- the parent commit of the change that
restructured fleet_amd/updater.py, checked out somewhere else:

    git worktree add --detach ../parent <parent commit>
    python tests/golden/make_updater_traces.py ../parent

Only that tree's fleet_amd/updater.py is read; what it imports from the package is the working
tree's. The file states the commit it was recorded from, and tests/test_updater_trace_cpu.py
holds the working tree's updater to it.
"""
import importlib.util
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import updater_trace  # noqa: E402


def main(tree: str) -> None:
    commit = subprocess.check_output(["git", "-C", tree, "rev-parse", "HEAD"], text=True).strip()
    dirty = subprocess.check_output(["git", "-C", tree, "status", "--porcelain", "fleet_amd/updater.py"], text=True)
    if dirty.strip():
        raise SystemExit(f"{tree}: fleet_amd/updater.py differs from {commit}")
    spec = importlib.util.spec_from_file_location("fleet_amd._reference_updater",
                                                  os.path.join(tree, "fleet_amd", "updater.py"))
    reference = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = reference  # (dataclasses looks the module up)
    spec.loader.exec_module(reference)
    records = updater_trace.run_all(reference)
    with open(os.path.join(HERE, "updater_traces.json"), "w") as f:  # one scenario per line
        f.write('{"recorded_from": "%s", "scenarios": {\n' % commit)
        f.write(",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in records.items()))
        f.write("\n}}\n")
    print(f"{len(records)} scenarios from {commit}")


if __name__ == "__main__":
    main(sys.argv[1])
