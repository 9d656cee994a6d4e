"""Out-of-sample confidence intervals on the batched engine (mirrors
mpisppy/confidence_intervals/): the Mak-Morton-Wood gap estimator (ciutils,
mmw_ci), the evaluation of a candidate on fresh samples (zhat4xhat) and the Bayraksan-Morton /
Bayraksan-Pierre-Louis sequential procedures (seqsampling).  Two-stage problems only: the
multistage parts of the reference (sample_tree.py, multi_seqsampling.py, EF_mstage), mmw_conf.py
and confidence_config.py are not served and raise NotImplementedError where a caller reaches them.
"""
