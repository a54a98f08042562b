"""Profiling switched on, and the counters reset, for the length of a ``with`` block on an engine."""


class Profiled:
    def __init__(self, e):
        self.e = e

    def __enter__(self):
        self.e.set_option("profile", 1)
        self.e.profile_reset()
        return self.e

    def __exit__(self, *exc):
        self.e.set_option("profile", 0)
