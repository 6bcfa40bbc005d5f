"""Every kernel instantiation of the built library, by name, for the census tests: one name per `__device_stub__` symbol
(hipcc emits one host stub per __global__ instantiation), spelled as rocprofv3 and hg_ctx_last_kernel spell it.

`nm -C` leaves a symbol mangled when its signature has a type the demangler does not know (a `_Float16 *` parameter:
prep_kernel, prep_fast_kernel, prep_cen_kernel).  Such a stub is read from its mangled form, `<length>__device_stub__<name>E`;
a mangled template instantiation, whose arguments could not be spelled, raises.  The number of names returned equals the
number of stub symbols: nothing is dropped silently."""
import re
import subprocess

STUB = "__device_stub__"
_DEMANGLED = re.compile(r"(?:::|\s|^)" + STUB + r"([A-Za-z_][A-Za-z_0-9]*(?:<[^>]*>)?)\(")
_MANGLED = re.compile(r"^_Z\w*?(\d+)" + STUB + r"(\w+)$")


def stub_name(symbol):
    """the kernel a stub symbol (demangled where nm could, mangled otherwise) stands for"""
    m = _DEMANGLED.search(symbol)
    if m:
        return m.group(1)
    m = _MANGLED.match(symbol.split()[-1])
    if not m:
        raise ValueError("a __device_stub__ symbol of unknown form: %r" % symbol)
    digits, rest = m.group(1), m.group(2)
    # (the enclosing name may end in a digit -- _GLOBAL__N_1 -- so the length is some suffix of the digits: the one that
    # leaves an identifier in front of the 'E' that closes the nested name)
    found = set()
    if symbol.split()[-1].startswith("_Z" + digits + STUB):  # at file scope: no nested name, the parameters follow directly
        length = int(digits) - len(STUB)
        if 1 <= length < len(rest) and rest[length] != "I":
            return rest[:length]
    for cut in range(len(digits)):
        length = int(digits[cut:]) - len(STUB)
        if digits[cut] != "0" and 1 <= length < len(rest) and rest[length] in "EI":
            found.add((rest[:length], rest[length]))
    if len(found) != 1 or next(iter(found))[1] != "E":
        raise ValueError("a mangled template (or otherwise unreadable) __device_stub__ symbol: %r" % symbol)
    return next(iter(found))[0]


def all_kernels(lib_path):
    """sorted list of the names of all kernel instantiations (a name twice: two stubs of one spelling)"""
    nm = subprocess.run(["nm", "-C", lib_path], capture_output=True, text=True, check=True).stdout
    names = []
    for line in nm.splitlines():
        if STUB not in line:
            continue
        parts = line.split(None, 2)  # address, type, symbol (an undefined symbol has no address: none is a stub)
        names.append(stub_name(parts[-1]))
    return sorted(names)


def family(name):
    """a kernel's name without its template arguments"""
    return name.split("<", 1)[0]
