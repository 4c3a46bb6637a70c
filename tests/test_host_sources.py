"""The host list of tests/host_sources.py against csrc/Makefile (CPU): the sanitizer legs build exactly the files of the
library that hold no kernel."""
import os
import re

from tests.host_sources import CSRC, HOST_SOURCES, makefile_sources


def test_every_makefile_source_is_host_code_or_holds_a_kernel():
    srcs = makefile_sources()
    assert len(srcs) == len(set(srcs)) and set(HOST_SOURCES) <= set(srcs), (srcs, HOST_SOURCES)
    for name in srcs:
        with open(os.path.join(CSRC, name)) as f:
            has_kernel = re.search(r"\b__global__\b", f.read()) is not None
        assert has_kernel != (name in HOST_SOURCES), \
            f"{name}: {'defines a kernel and is in HOST_SOURCES' if has_kernel else 'no kernel, and not in HOST_SOURCES'}"
