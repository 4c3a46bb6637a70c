"""What the compiler made of the int16-input kernels, read from the gfx950 code objects inside the built libsdrk.so (no GPU needed;
the extraction of tests/code_objects.py): the N = 4096 ci16 kernel keeps the complex64 flagship's budgets and really reads
4 bytes per sample, and neither the ci16 forms of fft_lds.hip nor the widening copy spill."""
import re
import subprocess

from tests.code_objects import OBJDUMP, code_objects, kernels, no_scratch as _no_scratch  # noqa: F401  (the fixtures)


def test_ci16_flagship_keeps_the_complex64_kernels_budgets(kernels):  # noqa: F811
    by = kernels
    hits = [k for n, k in by.items() if "fft4096_ci16_kernelILb" in n]
    assert len(hits) == 8, sorted(n for n in by if "ci16" in n)          # window on / off x both epilogues x both load forms
    for k in hits:
        assert k["vgpr_count"] <= 128, k
        assert k["group_segment_fixed_size"] <= 160 * 1024 // 3, k
        assert _no_scratch(k), k
    # the complex64 set the existing suite matches by "fft4096_kernelILb" is what it was
    assert len([n for n in by if "fft4096_kernelILb" in n]) == 4


def test_ci16_fft_lds_forms_and_the_unpack_kernel_do_not_spill(kernels):  # noqa: F811
    by = kernels
    # fft_lds_kernel<LOG2N, HAS_WINDOW, EPILOGUE, STAGED = false, CI16 = true>: LOG2N 8 ... 14 without 12, four forms each
    lds = {n: k for n, k in by.items() if re.search(r"fft_lds_kernelILi\d+ELb[01]ELi[01]ELb0ELb1EE", n)}
    lengths = sorted({int(re.search(r"fft_lds_kernelILi(\d+)E", n).group(1)) for n in lds})
    assert lengths == [8, 9, 10, 11, 13, 14], lengths
    assert len(lds) == 24, sorted(lds)
    for n, k in lds.items():
        assert _no_scratch(k), (n, k)
    unpack = [k for n, k in by.items() if "unpack_ci16_kernel" in n]
    synth = [k for n, k in by.items() if "synth_fill_ci16_kernel" in n]
    assert len(unpack) == 1 and len(synth) == 1
    assert _no_scratch(unpack[0]) and _no_scratch(synth[0])


def test_ci16_kernels_read_four_bytes_per_sample(code_objects):  # noqa: F811
    """The input loads of the N = 4096 ci16 kernel are dword loads (16 per thread and frame; direct form) or dwordx4 loads (4 per
    thread and frame; wide form), never dwordx2 as in the complex64 kernel, whose every buffer load is one; the widening copy
    keeps its 16-byte accesses although its rows are only 4-byte aligned."""
    loads = {}
    for co in code_objects:
        dis = subprocess.run([OBJDUMP, "-d", str(co)], check=True, capture_output=True, text=True).stdout
        cur = None
        for ln in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", ln)
            if m:
                cur = m.group(1) if "ci16" in m.group(1) or "fft4096_kernelILb1ELi0E" in m.group(1) else None
                if cur:
                    loads[cur] = []
            elif cur:
                m = re.search(r"\b((?:buffer|global|flat)_(?:load|store)_\w+)", ln)
                if m:
                    loads[cur].append(m.group(1))
    all_ops = {("fft4096_kernelILb1ELi0E" if "fft4096_kernelILb1ELi0E" in n else n): v for n, v in loads.items()}
    flagship = {n: v for n, v in loads.items() if "fft4096_ci16_kernelILb" in n}
    assert len(flagship) == 8
    for n, ops in flagship.items():
        ld = [o for o in ops if o.startswith("buffer_load")]           # the samples come through buffer loads (the global
        wide = bool(re.search(r"ELb1EEEv", n))                           # loads are the twiddle tables' and the window's)
        assert set(ld) == {"buffer_load_dwordx4" if wide else "buffer_load_dword"}, (n, ld)
        assert len(ld) >= (8 if wide else 32), (n, ld)                    # the first frame's loads and the prefetch's
    c64 = [o for o in all_ops["fft4096_kernelILb1ELi0E"] if o.startswith("buffer_load")]
    assert c64 and all(o == "buffer_load_dwordx2" for o in c64), c64
    unpack = next(v for n, v in loads.items() if "unpack_ci16_kernel" in n)
    assert "global_load_dwordx4" in unpack and unpack.count("global_store_dwordx4") >= 2, unpack
