"""No kernel of libdvbs2hip.so spills vector registers (VERDICT r2 found 15-17 spilled VGPRs in the SPA decoder, 6-11 in the register-resident
front ends, 8 in the shaping filter): read from the code objects' metadata (llvm-readelf --notes of every translation unit, tools/kernel_regs.py),
so it holds for the library that is in the tree, on CPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_no_kernel_spills_vector_registers():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no ROCm LLVM tools in this image")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from dvbs2_amd import build
    build.build_lib()
    import kernel_regs
    ks = kernel_regs.kernels()
    names = {k["name"] for k in ks}
    assert len(ks) >= 80 and any("ldpc_wg8_kernel<27, 4, 1>" in n for n in names) and any("ldpc_cu1_kernel<27, 3>" in n for n in names) and any("ldpc_wg8_kernel<27, 5, 0>" in n for n in names) and any("fir_mfma_kernel<2>" in n for n in names)
    assert not any("ldpc_fast2" in n for n in names), "stale object of a removed translation unit in dvbs2_amd/lib"
    bad = [(k["name"], k["vgpr_spill"]) for k in ks if k["vgpr_spill"] > 0]
    assert not bad, bad
    # private memory only where a kernel calls a non-inlined device function (the delay line's general walk)
    scratch = [(k["name"], k["scratch"]) for k in ks if k["scratch"] > 0]
    # ... and a 20-byte slot the backend reserves in the LDS-only min-sum kernels since their layer loop carries the address table's 28 registers (k_ldpc_wg8.hip, ATAB):
    # no instruction of the kernels touches it -- checked here in the disassembly -- so it is a frame-size entry, not a spill
    dead = [n for n, b in scratch if "ldpc_wg8_kernel<" in n and ", 0, 0>" in n and b <= 32]
    assert all("sync_vdelay_batch_kernel" in n or n in dead for n, _ in scratch), scratch
    if dead:
        import subprocess
        import kernel_mix as KM
        for name, ins in KM.functions(KM.disassemble("k_ldpc_wg8")).items():
            dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout
            if any(d in dem for d in dead):
                assert not [i for i in ins if i[1].startswith("scratch_") or "flat_scratch" in i[4]], dem


def test_no_kernel_calls_a_function_out_of_line():
    """Round 5: once ldpc_wg8_kernel had grown by the new output loops, the inliner left the constexpr helper w8_slot_lds out of line -- 80 calls per layer (s_swappc_b64 behind a
    waterfall loop each), the launch 3.7 times as long, every result still right.  The kernels are meant to be single functions: no call instruction in any code object."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("no ROCm LLVM tools in this image")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from dvbs2_amd import build
    build.build_lib()
    import glob
    import kernel_mix as KM
    bad, seen = [], 0
    for o in sorted(glob.glob(os.path.join(ROOT, "dvbs2_amd", "lib", "k_*.hip.o"))):
        tu = os.path.basename(o)[:-len(".hip.o")]
        for name, ins in KM.functions(KM.disassemble(tu)).items():
            seen += 1
            n = sum(1 for i in ins if i[1] in ("s_swappc_b64", "s_call_b64"))
            if n and "vd_source" not in name and "sync_vdelay_batch_kernel" not in name:      # (the delay line's general walk is a deliberate call: see the scratch note above)
                bad.append((tu, name, n))
    assert seen >= 80 and not bad, bad


def test_no_wide_buffer_store_takes_a_scalar_offset_register():
    """docs/negative_results.md: with an SGPR in the soffset field the compiler lets the next instruction overwrite the data registers of a 12- or 16-byte buffer store, and on gfx950 the
    stored data change.  The kernels put the whole offset into the vector register instead (`wide_off`); this reads the disassembly of every translation unit and wants no such store at
    all -- the stricter condition, so that the next edit of a store cannot bring the form back unseen -- and, as the hazard proper, none followed by a write of its data registers."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("no ROCm LLVM tools in this image")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from dvbs2_amd import build
    build.build_lib()
    import store_hazard
    rep = store_hazard.report()
    assert len(rep) >= 10 and rep["k_ldpc_wg8"][0] >= 40, rep        # the layer kernels do store 12 / 16 bytes at a time: the scan sees them
    assert not [(tu, bad) for tu, (_, _, bad) in rep.items() if bad], rep
    assert not [(tu, sgpr) for tu, (_, sgpr, _) in rep.items() if sgpr], rep


def test_layer_loop_instruction_mix_is_read_from_the_code_object():
    """tools/kernel_mix.py prices a kernel's vector instructions by class (profiles/r04_probe_issue.txt: 2.07 SIMD cycles for the simple two-operand class -- v_mov / v_and / v_or / v_xor /
    v_add / v_sub / v_mul with register or inline operands --, 2.6 the same with a literal, 4.2-4.25 everything else: VOP3 / VOP3P / SDWA / DPP encodings, SGPR or vcc operands, VOPC, v_min /
    v_max / shifts / conversions / v_fmac; 8.06 transcendental); bench.py's roofline.bounded.valu and the profile summaries multiply SQ_INSTS_VALU by that price.  The min-sum layer loop
    is made of the expensive kind: nearly half of it VOP3-encoded, under a tenth of it in the simple class, 3.8 .. 4.1 cycles per instruction; no transcendental in it."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_mix as KM
    from dvbs2_amd import build
    build.build_lib()
    cpi, how = KM.price_kernel("ldpc_wg8_kernel<27,5>")
    assert how["scope"] == "layer loop" and how["mix"]["trans"] == 0 and 3.8 < cpi < 4.1, (cpi, how)
    n = sum(how["mix"].values())
    assert 500 < n < 800 and 0.40 < how["mix"]["vop3"] / n < 0.55 and how["mix"]["plain"] / n < 0.12
    cpi_spa, how_spa = KM.price_kernel("ldpc_wg8_kernel<27,0,1>")
    assert how_spa["mix"]["trans"] >= 100 and cpi_spa < cpi + 0.5
