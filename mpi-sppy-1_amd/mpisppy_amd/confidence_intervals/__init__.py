"""Out-of-sample confidence intervals on the batched engine (mirrors
mpisppy/confidence_intervals/): the Mak-Morton-Wood gap estimator (ciutils,
mmw_ci), the evaluation of a candidate on fresh samples (zhat4xhat) and the Bayraksan-Morton /
Bayraksan-Pierre-Louis sequential procedures (seqsampling).  Multistage problems:
sample_tree (SampleSubtree, walking_tree_xhats) and the gap estimators and MMW interval with
EF_mstage, every stage's subtrees solved at once as one conditioned tree extensive form.  Not
served, raising NotImplementedError where a caller reaches them: zhat4xhat.evaluate_sample_trees,
multi_seqsampling.py and SeqSampling with EF_mstage; mmw_conf.py and confidence_config.py belong to
the CLI/config system.
"""
