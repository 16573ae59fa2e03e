"""The Python surface of ``fleet_amd`` is what it was before the package file was split.

``api_surface.json`` beside this file was recorded on the commit before the split, with this
file's own ``surface()``::

    import json, fleet_amd, test_api_surface as t
    json.dump(t.surface(fleet_amd), open("tests/api_surface.json", "w"), indent=1, sort_keys=True)

It holds the package's public names (the 50 of its 54 that are no module) with the six private ones that
tests and scripts reach, and for every class each member that is a function, property or staticmethod (232, and FleetError's
constructor once more under each of its two subclasses):
its kind, ``str(inspect.signature(...))`` and the SHA-1 of ``inspect.getdoc(...)``.

What the test holds the package to:

* every recorded name is still there, but for the six incidental imports of the old file
  (``C``, ``np``, ``os``, ``Optional``, ``Sequence``, ``annotations``), and there is no new
  one but the modules the file was split into;
* every recorded member a user can call -- public or dunder -- is there with the same kind,
  signature and docstring, and no class has a new public member but the lifecycle the handle
  base gives it;
* a recorded private member keeps kind and signature, or is one of the two copies that the
  shared helpers replaced (``GONE``). The docstring of a private member is not surface:
  ``Gate._live`` and ``Ledger._live`` are now the base's.

No library is loaded and no GPU is needed.
"""
import hashlib
import inspect
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "api_surface.json")
PRIVATE = ("_as_bytes", "_stream", "_ptr", "_eval_host_args", "_eval_host_call", "_eval_device_out")
INCIDENTAL = {"C", "np", "os", "Optional", "Sequence", "annotations"}
LIFECYCLE = {"close", "__del__", "__enter__", "__exit__"}
GONE = {("Accumulator", "_burst_args"), ("KardamFilter", "_check_tensors")}


def _member(v):
    f = v.fget if isinstance(v, property) else v.__func__ if isinstance(v, staticmethod) else v
    doc = inspect.getdoc(f)
    return [type(v).__name__, str(inspect.signature(f)), None if doc is None else hashlib.sha1(doc.encode()).hexdigest()]


def surface(pkg):
    # (submodules and the lazy ACC_BURST appear in the namespace as they are first used: not recorded)
    names = sorted(n for n, v in vars(pkg).items()
                   if not n.startswith("_") and not inspect.ismodule(v) and n != "ACC_BURST")
    classes = {}
    for n in names:
        c = vars(pkg)[n]
        if not inspect.isclass(c):
            continue
        members = {}
        for base in reversed(c.__mro__[:-1]):  # the class and its bases, the nearest definition last
            for k, v in vars(base).items():
                if inspect.isfunction(v) or isinstance(v, (property, staticmethod)):
                    members[k] = _member(v)
        classes[n] = members
    return {"names": names, "private": sorted(p for p in PRIVATE if hasattr(pkg, p)), "classes": classes}


def _private(name):
    return name.startswith("_") and not name.startswith("__")


def test_surface_is_the_recorded_one():
    sys.path.insert(0, ROOT)
    import fleet_amd
    want, got = json.load(open(RECORD)), surface(fleet_amd)
    assert set(want["names"]) - set(got["names"]) <= INCIDENTAL
    assert set(got["names"]) <= set(want["names"])
    assert got["private"] == want["private"] == sorted(PRIVATE)
    assert sorted(got["classes"]) == sorted(want["classes"])
    for cls, members in want["classes"].items():
        now = got["classes"][cls]
        for name, rec in members.items():
            if _private(name):
                assert (cls, name) in GONE or now[name][:2] == rec[:2], (cls, name)
            else:
                assert now[name] == rec, (cls, name, now.get(name), rec)
        new_public = {k for k in set(now) - set(members) if not _private(k)}
        assert new_public <= LIFECYCLE, (cls, new_public)


def test_import_stays_lazy():
    """Importing the package loads neither torch nor the library; ACC_BURST loads it when asked."""
    code = ("import sys, fleet_amd, fleet_amd._capi as K\n"
            "assert 'torch' not in sys.modules, 'torch imported'\n"
            "assert K._lib is None, 'library loaded'\n"
            "import os\n"
            "if os.path.exists(fleet_amd.LIB_PATH):\n"
            "    assert fleet_amd.ACC_BURST == fleet_amd.lib().fleet_acc_burst()\n"
            "    assert K._lib is not None\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
