"""A recording stand-in for the kernel library (``program.lib`` is a plain attribute)."""
from __future__ import annotations

_QUERY_SUFFIXES = ("_splits", "_slabs", "_nslab", "_ws", "_ok", "_rows", "_grid")


class Recorder:
    """Wraps the ctypes library: records (name, fn, args) of every csa_* call.  ``queries``:
    the plan-time questions, the profile setters and the flag getters too (a timing replay
    wants launches only; a launch trace wants every call)."""

    def __init__(self, lib, queries: bool = False):
        self.lib = lib
        self.queries = queries
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith("csa_"):
            return fn
        if not self.queries and (name.endswith(_QUERY_SUFFIXES) or name.startswith("csa_set_")
                                 or name in ("csa_deterministic", "csa_packed")):
            return fn

        def wrapped(*args):
            self.calls.append((name, fn, args))
            return fn(*args)
        return wrapped
