"""The C-ABI library on the CPU (no GPU, no compute calls): it loads, exports every entry point include/srgan_hip.h
declares (and the ctypes table binds exactly those, with the header's argument and field types), reports its
capabilities, refuses a stale build, and rejects bad arguments before touching a device."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'srgan_hip.h')


def header_code():
    """include/srgan_hip.h without comments and preprocessor lines (a `#define` or `#endif` is not a return type)."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', '', open(HEADER).read(), flags=re.DOTALL)
    return re.sub(r'^\s*#[^\n]*', '', text, flags=re.MULTILINE)


def header_structs():
    """{struct name: [(field, class)]} of the header's typedef'd structs; an array field's class is e.g. 'char[16]'."""
    structs = {}
    for name, body in re.findall(r'typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\w+\s*;', header_code(), flags=re.DOTALL):
        fields = structs[name] = []
        for declaration in body.split(';')[:-1]:
            c_type, names = re.fullmatch(r'\s*(.+?[\s*])(\w+(?:\[\d+\])?(?:\s*,\s*\w+)*)\s*', declaration).groups()
            for field in names.split(','):
                array = re.fullmatch(r'\s*(\w+)\[(\d+)\]', field)
                fields.append((array[1], '%s[%s]' % (c_type.strip(), array[2])) if array else (field.strip(), c_class(c_type)))
    return structs


def header_prototypes():
    """{entry point: (C return type, [C argument types])} of every function the header declares."""
    code = re.sub(r'typedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;', '', header_code(), flags=re.DOTALL)
    code = re.sub(r'extern\s+"C"\s*\{|\}', '', code)
    prototypes = {}
    for statement in code.split(';'):
        match = re.fullmatch(r'\s*(.*?[\s*])(srgan_\w+)\s*\((.*)\)\s*', statement, flags=re.DOTALL)
        if match:
            arguments = [' '.join(a.split()) for a in match.group(3).split(',')]
            arguments = [re.sub(r'\s*\b\w+$', '', a) if re.search(r'[\w*]\s+\w+$', a) else a for a in arguments]
            prototypes[match.group(2)] = (' '.join(match.group(1).split()), [] if arguments == ['void'] else arguments)
    return prototypes


def declared_entry_points():
    return sorted(header_prototypes())


def c_class(c_type):
    """pointer / i32 / i64 / f32 / f64 of a C type from the header (signedness is not compared)."""
    if '*' in c_type:
        return 'pointer'
    c_type = c_type.replace('const ', '').strip()
    classes = {'int': 'i32', 'int32_t': 'i32', 'uint32_t': 'i32', 'int64_t': 'i64', 'float': 'f32', 'double': 'f64'}
    return classes[c_type]


def ctypes_class(c_type):
    if c_type in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(c_type, ctypes._Pointer):
        return 'pointer'
    if c_type in (ctypes.c_float, ctypes.c_double):
        return 'f%d' % (8 * ctypes.sizeof(c_type))
    assert issubclass(c_type, ctypes._SimpleCData) and c_type._type_ in 'bBhHiIlLqQ', c_type
    return 'i%d' % (8 * ctypes.sizeof(c_type))


@pytest.fixture(scope='module')
def lib():
    import srgan_amd  # noqa: F401
    from srgan_amd import _lib
    return _lib


def test_every_declared_entry_point_is_exported_and_bound(lib):
    from srgan_amd import _build
    declared = declared_entry_points()
    assert len(declared) >= 45
    exported = subprocess.run(['nm', '-D', '--defined-only', _build.LIBRARY], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(re.findall(r'\bT (srgan_[a-z0-9_]+)$', exported, flags=re.MULTILINE)))
    assert exported == declared, (sorted(set(declared) - set(exported)), sorted(set(exported) - set(declared)))
    assert sorted(lib.SIGNATURES) == declared           # the Python binding covers the whole ABI
    library = lib.library()
    for name in declared:
        assert getattr(library, name) is not None


def test_the_ctypes_table_matches_the_header_prototypes(lib):
    """Every SIGNATURES entry has the header's argument count, argument classes and return class; a pointer to one of the
    mirrored structs points to the struct the header names."""
    prototypes = header_prototypes()
    assert len(prototypes) == len(set(re.findall(r'\b(srgan_\w+)\s*\(', header_code())))       # no declaration skipped
    mirrors = {lib.ConvDesc: 'srgan_conv_desc', lib.BnRelu: 'srgan_bn_relu', lib.BnReduceJob: 'srgan_bn_reduce_job',
               lib.Capabilities: 'srgan_capabilities_t'}
    for name, (argtypes, restype) in lib.SIGNATURES.items():
        c_return, c_arguments = prototypes[name]
        assert len(argtypes) == len(c_arguments), (name, len(argtypes), c_arguments)
        for position, (binding, declared) in enumerate(zip(argtypes, c_arguments)):
            assert ctypes_class(binding) == c_class(declared), (name, position, binding, declared)
            if getattr(binding, '_type_', None) in mirrors:
                assert re.sub(r'\bconst\s+|\s*\*$', '', declared) == mirrors[binding._type_], (name, position, declared)
        assert ctypes_class(restype) == c_class(c_return), (name, restype, c_return)


def test_the_struct_mirrors_match_the_header(lib):
    """Field names, order and widths of the ctypes.Structure mirrors against the header's structs."""
    structs = header_structs()
    mirrors = {'srgan_conv_desc': lib.ConvDesc, 'srgan_bn_relu': lib.BnRelu, 'srgan_bn_reduce_job': lib.BnReduceJob,
               'srgan_capabilities_t': lib.Capabilities}
    assert sorted(structs) == sorted(mirrors)
    for name, mirror in mirrors.items():
        bound = [(field, 'char[%d]' % ctypes.sizeof(t) if issubclass(t, ctypes.Array) else ctypes_class(t))
                 for field, t in mirror._fields_]
        assert bound == structs[name], (name, bound, structs[name])


def test_capabilities_and_build_identity(lib):
    from srgan_amd import _build
    caps = lib.capabilities()
    assert caps.abi_version == lib.library().srgan_version() == 110
    assert caps.struct_bytes == ctypes.sizeof(lib.Capabilities) and caps.arch == b'gfx950'
    assert caps.dtypes == 0x7 and caps.features & 0x7 == 0x7
    assert caps.workspace_bytes == lib.library().srgan_workspace_bytes() == 256 << 20      # (round 5: the partial tiles of every K split)
    assert caps.max_tensor_elements == 2 ** 31 - 1
    assert lib.library().srgan_build_id().decode() == _build.source_id() == _build.library_id()
    assert lib.library().srgan_capabilities(None, 0) == lib.EINVAL


def test_a_library_built_from_other_sources_is_refused(lib, monkeypatch):
    """a stale prebuilt .so must not run silently -- the loader compares the source id compiled into the
    library with the kernel sources next to it."""
    monkeypatch.setattr(lib, '_library', None)
    monkeypatch.setattr(lib, 'source_id', lambda: '0123456789abcdef')
    monkeypatch.delenv('SRGAN_ALLOW_STALE_LIBRARY', raising=False)
    with pytest.raises(lib.HipLibraryError, match='other kernel sources'):
        lib.library()


def test_argument_errors_are_reported_before_any_device_work(lib):
    library = lib.library()
    huge = lib.ConvDesc(4096, 512, 1024, 1024, 64, 3, 3, 1, 1, 1, 1, 1024, 1024, 0, 0, 0)        # 2^41 input elements
    assert library.srgan_conv2d_fwd(ctypes.byref(huge), 16, 16, None, 16, 0, None) == lib.ERANGE
    assert b'2^31' in library.srgan_last_error()
    malformed = lib.ConvDesc(1, 8, 8, 8, 8, 3, 3, 0, 1, 1, 1, 8, 8, 0, 0, 0)                       # stride 0
    assert library.srgan_conv2d_fwd(ctypes.byref(malformed), 16, 16, None, 16, 0, None) == lib.EINVAL
    wrong_dtype = lib.ConvDesc(1, 8, 8, 8, 8, 3, 3, 1, 1, 1, 1, 8, 8, 0, 0, 7)
    assert library.srgan_conv2d_fwd(ctypes.byref(wrong_dtype), 16, 16, None, 16, 0, None) == lib.EINVAL
    assert library.srgan_conv2d_bnrelu_supported(ctypes.byref(huge), 0) == 0
    assert library.srgan_set_workspace(16, 1024, None) == lib.EINVAL                              # smaller than required
    assert library.srgan_set_workspace(8, 256 << 20, None) == lib.EINVAL                          # misaligned
    # the RCCL entry points check their arguments before they resolve / reach RCCL
    assert library.srgan_comm_unique_id(None) == lib.EINVAL
    assert library.srgan_comm_init(None, 1, 0, None) == lib.EINVAL
    holder = ctypes.c_void_p()
    assert library.srgan_comm_init(ctypes.byref(holder), 2, 2, b'\0' * 128) == lib.EINVAL          # rank outside the world
    assert library.srgan_all_reduce_sum(None, 16, 16, 4, 0, None) == lib.EINVAL
    assert library.srgan_reduce_scatter_sum(16, 16, 16, 4, 5, None) == lib.EINVAL                 # unknown wire dtype
    assert library.srgan_comm_available() in (0, 1)
