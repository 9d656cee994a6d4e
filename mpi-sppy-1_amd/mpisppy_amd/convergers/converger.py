"""Base class of the converger objects (mirrors mpisppy/convergers/converger.py:18-41).

PHBase constructs ``ph_converger(ph)`` at the end of Iter0 and asks ``is_converged()`` once
per iteration, after ``miditer`` (phbase.py:919-926); a user-supplied converger does not
compute ``ph.conv``.
"""
import abc


class Converger:
    # converger.py:24-25
    def __init__(self, opt):
        self.conv = None  # the value used for the comparison

    # converger.py:27-35
    @abc.abstractmethod
    def is_converged(self):
        """True ends the loop at the current iteration: no more solves."""

    # converger.py:37-41
    def post_loops(self):
        """Called after the loop, after the extensions' post_loops."""
