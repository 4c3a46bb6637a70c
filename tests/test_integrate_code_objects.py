"""What the compiler made of the integrated-spectrum kernels, read from the gfx950 code objects inside the built libsdrk.so (no
GPU needed; the extraction of tests/code_objects.py): the N = 4096 kernel with its 16 or 32 accumulators still fits three
workgroups per CU — at most 168 VGPRs, a third of the LDS, no scratch — and the scalar unit of the new kernels does nothing
to memory but load from it."""
import re
import subprocess

from tests.code_objects import OBJDUMP, code_objects, kernels, no_scratch as _no_scratch  # noqa: F401  (the fixtures)


# Everything the scalar unit may do in these kernels, as an allow-list: arithmetic / logic / compares / moves (typed suffix),
# loads, and program control.  Anything else on the scalar unit — any way of writing memory from it included — fails the test.
SCALAR_ALU = re.compile(r"^s_\w+_(?:b32|b64|i32|u32|i64|u64|b16|i16|u16)$")
SCALAR_LOAD = re.compile(r"^s_(?:buffer_)?load_dword(?:x\d+)?$")
SCALAR_CONTROL = re.compile(r"^s_(?:waitcnt\w*|barrier|branch|cbranch_\w+|endpgm|nop|code_end|sleep|setprio|sendmsg\w*)$")


def test_the_4096_kernel_fits_three_workgroups_per_cu(kernels):  # noqa: F811
    by = kernels
    hits = {n: k for n, k in by.items() if "fft4096_integrate_kernelILb" in n}
    assert len(hits) == 6, sorted(hits)                                    # window on / off x mean / max / min
    for n, k in hits.items():
        assert k["vgpr_count"] <= 168, (n, k)
        assert k["group_segment_fixed_size"] == (53376 if "ILb1E" in n else 36992), (n, k)   # exchange + tables (+ window)
        assert k["group_segment_fixed_size"] <= 160 * 1024 // 3, (n, k)
        # no scratch memory and no vector register spilled (the unit bookkeeping overflows the scalar file by a dozen values,
        # which the compiler parks in the lanes of a vector register it has to spare: no memory behind that)
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (n, k)
        assert k.get("sgpr_spill_count", 0) <= 16, (n, k)               # 13-14 today: seen if it grows
    # the compensation is what the mean pays over max / min: more registers, not a spill
    mean = max(k["vgpr_count"] for n, k in hits.items() if "ELi0EE" in n)
    hold = max(k["vgpr_count"] for n, k in hits.items() if "ELi0EE" not in n)
    assert hold < mean, (hold, mean)
    # and the per-frame kernels the existing suite counts are what they were
    assert len([n for n in by if "fft4096_kernelILb" in n]) == 4


def test_the_generic_route_and_finalize_do_not_spill(kernels):  # noqa: F811
    by = kernels
    rows = [k for n, k in by.items() if "integrate_rows_kernel" in n]
    fin = [k for n, k in by.items() if "integrate_finalize_kernel" in n]
    assert len(rows) == 3 and len(fin) == 1
    assert all(_no_scratch(k) for k in rows + fin)


def test_the_scalar_unit_only_computes_loads_and_branches(code_objects):  # noqa: F811
    kernels, seen = set(), set()
    for co in code_objects:
        dis = subprocess.run([OBJDUMP, "-d", str(co)], check=True, capture_output=True, text=True).stdout
        cur = None
        for ln in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", ln)
            if m:
                cur = m.group(1) if "integrate" in m.group(1) else None
                if cur:
                    kernels.add(cur)
                continue
            m = re.match(r"^\s+(s_\w+)", ln) if cur else None
            if m:
                op = m.group(1)
                seen.add(op)
                assert SCALAR_ALU.match(op) or SCALAR_LOAD.match(op) or SCALAR_CONTROL.match(op), (cur, ln.strip())
    assert len(kernels) == 10, sorted(kernels)
    assert any(SCALAR_LOAD.match(op) for op in seen)                    # (the kernel arguments: the pattern does see the unit)
