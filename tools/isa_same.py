"""Are the kernels of two builds the same device code?  Reads the gfx950 code objects out of two `lib` directories (dvbs2_amd/lib of two checkouts, each built by
dvbs2_amd/build.py), disassembles every object whose name matches OBJECTS (a glob without the .hip.o; default k_ldpc*, the LDPC kernels; 'k_*' is every kernel file) and
compares each function's instruction text (mnemonic and operands; addresses and encodings left out) by symbol name -- a symbol may have moved to another translation
unit.  No GPU.  It compares text only and looks for no particular instruction.
usage: python tools/isa_same.py OLD_LIB_DIR NEW_LIB_DIR [OBJECTS]      -> one line per symbol: equal / DIFFERENT / only in ...; exit status 1 unless all are equal"""
import glob, os, sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_mix as KM


def symbols(libdir, objects):
    """demangled-as-is symbol -> (translation unit, [(mnemonic, operands)])"""
    out = {}
    pattern = objects if objects.endswith(".hip.o") else objects + ".hip.o"
    for o in sorted(glob.glob(os.path.join(libdir, pattern))):
        tu = os.path.basename(o)[:-len(".hip.o")]
        for name, insts in KM.functions(KM.disassemble_object(o)).items():
            out[name] = (tu, [(i[1], i[4].strip()) for i in insts])
    return out


def main():
    objects = sys.argv[3] if len(sys.argv) > 3 else "k_ldpc*"
    old, new = symbols(sys.argv[1], objects), symbols(sys.argv[2], objects)
    bad = 0
    print("| symbol | instructions | old file | new file | device code |\n|---|---|---|---|---|")
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            verdict = "only in " + ("old" if name in old else "new"); bad += 1
        elif old[name][1] == new[name][1]:
            verdict = "equal"
        else:
            first = next((k for k, (a, b) in enumerate(zip(old[name][1], new[name][1])) if a != b), min(len(old[name][1]), len(new[name][1])))
            verdict = "DIFFERENT (from instruction %d)" % first; bad += 1
        print("| `%s` | %d | %s | %s | %s |" % (name, len((new if name in new else old)[name][1]), old.get(name, ("-",))[0], new.get(name, ("-",))[0], verdict))
    print("\n%d symbols, %d not equal" % (len(set(old) | set(new)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
