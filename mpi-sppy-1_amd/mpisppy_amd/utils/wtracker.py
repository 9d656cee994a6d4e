"""WTracker.W_diff: the dual metric of the gradient rho extension (mirrors
mpisppy/utils/wtracker.py:134-157).  Only this method: the moving-window reports
(compute_moving_stats, report_by_moving_stats) keep every iteration's W on the host and are
not carried over.
"""


class WTracker:
    def __init__(self, PHB):
        self.PHB = PHB

    def W_diff_device(self):
        """Enqueue the metric (engine.w_diff -> phgpu_w_diff and the ranks' sum); returns the
        device double[2] {previous, current} without reading anything back."""
        return self.PHB.engine.w_diff()

    def W_diff(self):
        """The mean |W - W of the previous call| over all scenarios and nonants (host float);
        0 at the first call, as the reference's local_Ws[-1] = local_Ws[0] (wtracker.py:143).
        With several ranks this departs from wtracker.py:155-157: the reference divides the sum
        of the ranks' own means by n_proc, here every rank's mean is weighted by its share of
        the scenarios, so the value does not depend on the split (equal for an even split)."""
        self.W_diff_device()
        return self.PHB.engine.w_diff_value()
