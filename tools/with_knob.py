"""Run a script of the repository with the library's debug knobs set (pvo_debug_config is process-wide and not an environment
variable, so a measurement of a knob needs the knob set inside the measuring process):
    python tools/with_knob.py edge_blocks=third+low [knob=value ...] bench.py [bench.py arguments]
    python tools/with_knob.py edge_blocks=half tools/update_poison_check.py
    python tools/with_knob.py edge_blocks=half+agg+trunk bench.py          (the trunk per block of edges as well)
The script runs as __main__ in this process, with the product library (or, lib=<tag>, a tools/variant.py build)."""
import os, runpy, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
args = sys.argv[1:]
from pvo_amd import _lib, droid_backends as db      # noqa: E402
while args and "=" in args[0] and not args[0].endswith(".py"):
    k, v = args.pop(0).split("=", 1)
    if k == "lib":
        _lib.LIB_PATH = os.path.join(ROOT, "tools", "_probe", "libpvo_hip_%s.so" % v)
    else:
        db.debug_config(k, v if not v.lstrip("-").isdigit() else int(v))
script = args[0] if os.path.isabs(args[0]) else os.path.join(ROOT, args[0])
sys.argv = [script] + args[1:]
sys.path.insert(0, os.path.dirname(script))
runpy.run_path(script, run_name="__main__")
