"""tests/host/request_harness.cpp built with AddressSanitizer and UndefinedBehaviorSanitizer (host_harness.build, sanitize=True)
and run on the lines of tests/test_request_host.py: a stand-alone program, nothing is preloaded.  No GPU."""
from tests import request_util as ru
from tests import test_request_host as host


def test_harness_is_clean_under_the_sanitizers(tmp_path):
    exe = ru.build_harness(tmp_path, sanitize=True)
    host.check_vertices(exe)
    host.check_limits(exe)
    host.check_backward(exe)
