"""The evaluation side of the package, module for module the reference's ``balf/benchmark_test``.

The record constructors of the HSequences / GoPro evaluation, ``create_results`` and ``create_metrics_results``, are defined in
:mod:`.metrics_results` and published here under the reference's module name as well, so that
``from balf_amd.benchmark_test.test_utils import create_metrics_results`` works as the reference's import does."""
from . import metrics_results, test_utils

test_utils.RESULT_KEYS = metrics_results.RESULT_KEYS
test_utils.create_results = metrics_results.create_results
test_utils.create_metrics_results = metrics_results.create_metrics_results
