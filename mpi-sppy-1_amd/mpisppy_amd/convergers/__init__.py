"""Convergers of the PH loop (mirrors mpisppy/convergers/): norm-rho and primal-dual."""
