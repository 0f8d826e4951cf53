"""The result record of the HSequences / GoPro evaluation (reference balf/benchmark_test/test_utils.py:5-28): a plain dict,
with the reference's field names.  The reference declares the fields; ``evaluate.evaluate_matching_hsequences`` fills them
(repeatability and matching score).  The package publishes both constructors as
``benchmark_test.test_utils.create_results`` / ``create_metrics_results`` too, the reference's import path
(``benchmark_test/__init__.py``); the resize protocol's records are defined in ``benchmark_test.test_utils`` itself."""

RESULT_KEYS = ('num_features', 'rep_single_scale', 'rep_multi_scale', 'num_points_single_scale', 'num_points_multi_scale',
               'error_overlap_single_scale', 'error_overlap_multi_scale', 'mma', 'mma_corr', 'num_matches', 'num_mutual_corresp',
               'avg_mma')


def create_results():
    """One empty list per field."""
    return {k: [] for k in RESULT_KEYS}


def create_metrics_results(sequences, top_k, overlap, pixel_threshold):
    results = create_results()
    results['sequences'] = sequences
    results['top_k'] = top_k
    results['overlap'] = overlap
    results['pixel_threshold'] = pixel_threshold
    return results
