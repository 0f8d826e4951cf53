"""The result records of the resize protocol (reference balf/benchmark_test/test_utils.py:31-46): plain dicts."""

RESIZE_RESULT_KEYS = ('repeatability', 'localization_err', 'common_src_num', 'common_dst_num', 'rep_src_num', 'rep_dst_num')


def create_reisze_results():
    """(The reference's spelling.)  One empty list per field of ``compute_resize_repeatability``'s dict."""
    return {k: [] for k in RESIZE_RESULT_KEYS}


def create_resize_metrics_results(sequences, top_k, pixel_threshold):
    results = create_reisze_results()
    results['sequences'] = sequences
    results['top_k'] = top_k
    results['pixel_threshold'] = pixel_threshold
    return results
