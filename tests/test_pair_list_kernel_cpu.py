"""Register budget of the pair-list kernels (csrc/pair_list.hip), read from the gfx950 code object in the product library.
The kernel waits for memory, so every form must run without scratch and without LDS.  The forms that keep the row's planes
in registers request a whole partner (up to 3 x 3.5 KB per wave) at once: 4 waves per SIMD (<= 128 VGPRs) keep 10-40 KB
per SIMD in flight.  The stepped forms hold two steps (the current and the requested one: 4 x 14 registers) and keep one
step of 3.5 KB per wave in flight: at 8 TB/s and ~2 us that takes 16 MB over 1 024 SIMDs, i.e. 5 waves per SIMD
(<= 96 VGPRs)."""
import re

from test_capi_cpu import _kernel_metadata


def test_register_budget_of_the_pair_list_kernels():
    import sketchlib.rust_amd as pkg

    pkg.build_library()
    meta = _kernel_metadata(pkg.library_path())
    forms = {k: v for k, v in meta.items() if "pair_list_kernel<" in k}
    # one, two or three flat trips with the row's planes kept; the stepped form; the stepped form with counts to memory
    want = {(1, "false"), (2, "false"), (3, "false"), (0, "false"), (0, "true")}
    seen = set()
    for name, (vgpr, scratch, lds) in forms.items():
        ft, counts_out = re.search(r"pair_list_kernel<(\d+), (true|false)>", name).groups()
        seen.add((int(ft), counts_out))
        assert scratch == 0 and lds == 0, (name, scratch, lds)
        assert vgpr <= (96 if ft == "0" else 128), (name, vgpr)
    assert seen == want and len(forms) == len(want), sorted(forms)
    (vgpr, scratch, lds), = [v for k, v in meta.items() if "pair_list_fit_kernel" in k]
    assert scratch == 0 and lds == 0 and vgpr <= 128, (vgpr, scratch, lds)
