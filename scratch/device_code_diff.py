#!/usr/bin/env python3
"""Per-symbol comparison of the gfx950 device code of two builds of libsrgan_hip.so.

    python scratch/device_code_diff.py PARENT.so RESULT.so

From each library: the .hip_fatbin section (llvm-objcopy), split at every __CLANG_OFFLOAD_BUNDLE__ header, the
hipv4-amdgcn-amd-amdhsa--gfx950 entry of each bundle written out as a code object.  Per code object every defined FUNC
symbol with its size (llvm-readelf -s -W) and its disassembly (llvm-objdump -d --no-show-raw-insn), cut at the symbol's
size (the s_nop padding behind a code object's last symbol is not its code) with the addresses stripped; and, per
kernel, .vgpr_count / .group_segment_fixed_size / .private_segment_fixed_size from the code object's metadata
(llvm-readelf --notes).  Prints the counts, the symbols found in only one library, and name, sizes and resource
figures of every symbol that differs.  Exit status 1 when anything differs.  Needs the LLVM tools of a ROCm
installation (ROCM_PATH, default /opt/rocm); no GPU."""
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin')
MAGIC = b'__CLANG_OFFLOAD_BUNDLE__'
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'
RESOURCES = ('.vgpr_count', '.agpr_count', '.sgpr_count', '.group_segment_fixed_size', '.private_segment_fixed_size')


def tool(name, *arguments):
    return subprocess.run([os.path.join(LLVM, name), *arguments], check=True, capture_output=True).stdout


def code_objects(library, directory):
    """The gfx950 code objects of the library's fat binary, as files under `directory`."""
    section = os.path.join(directory, 'fatbin')
    tool('llvm-objcopy', '-O', 'binary', '--only-section=.hip_fatbin', library, section)
    with open(section, 'rb') as handle:
        blob = handle.read()
    paths, at = [], blob.find(MAGIC)
    while at >= 0:
        following = blob.find(MAGIC, at + 1)
        bundle = blob[at:following if following >= 0 else len(blob)]
        (entries,) = struct.unpack_from('<Q', bundle, len(MAGIC))
        cursor = len(MAGIC) + 8
        for _ in range(entries):
            offset, size, length = struct.unpack_from('<QQQ', bundle, cursor)
            triple = bundle[cursor + 24:cursor + 24 + length].decode()
            cursor += 24 + length
            if triple == TARGET and size:
                paths.append(os.path.join(directory, 'code_object_%d.co' % len(paths)))
                with open(paths[-1], 'wb') as handle:
                    handle.write(bundle[offset:offset + size])
        at = following
    return paths


def symbols_of(code_object):
    """{mangled name: (size, instruction text)} of every defined FUNC symbol, and {kernel name: resource figures}."""
    sized = {}
    for line in tool('llvm-readelf', '-s', '-W', code_object).decode().splitlines():
        fields = line.split()
        if len(fields) == 8 and fields[3] == 'FUNC' and fields[6] != 'UND':
            sized[fields[7]] = (int(fields[1], 16), int(fields[2]))
    by_address = {address: name for name, (address, _) in sized.items()}
    text, current, limit = {name: [] for name in sized}, None, 0
    for line in tool('llvm-objdump', '-d', '--no-show-raw-insn', code_object).decode().splitlines():
        label = re.match(r'^([0-9a-f]+) <(.+)>:$', line)
        if label:
            current = by_address.get(int(label.group(1), 16))
            limit = sum(sized[current]) if current else 0
            continue
        instruction = re.match(r'^\s+(.*?)\s*// ([0-9A-Fa-f]+):', line)
        if current and instruction and int(instruction.group(2), 16) < limit:
            text[current].append(re.sub(r'\s+', ' ', instruction.group(1)))
    resources, kernel, depth = {}, None, None
    for line in tool('llvm-readelf', '--notes', code_object).decode().splitlines():
        if line.strip() == 'amdhsa.kernels:':
            depth = len(line) - len(line.lstrip()) + 2         # the list's entries; a kernel's .args list sits deeper
            continue
        entry = re.match(r'^(\s*)(- )?(\.[a-z_]+):\s*(\S+)', line)
        if depth is None or not entry:
            continue
        if entry.group(2) and len(entry.group(1)) == depth:
            kernel = {}
        if kernel is not None and len(entry.group(1)) - (0 if entry.group(2) else 2) == depth:
            if entry.group(3) in RESOURCES:
                kernel[entry.group(3)] = entry.group(4)
            if entry.group(3) == '.name':
                resources[entry.group(4).strip("'\"")] = kernel
    return {name: (sized[name][1], '\n'.join(text[name])) for name in sized}, resources


def library_symbols(library):
    with tempfile.TemporaryDirectory() as directory:
        objects = code_objects(library, directory)
        symbols, resources = {}, {}
        for code_object in objects:
            found, figures = symbols_of(code_object)
            for name, value in found.items():
                # (a weak device function instantiated in several translation units: one entry per copy)
                symbols.setdefault(name, []).append(value)
            resources.update(figures)
    return len(objects), {name: sorted(copies) for name, copies in symbols.items()}, resources


def demangled(names):
    """Readable names where a demangler is installed (llvm-cxxfilt of the ROCm tree, else binutils' c++filt), else as they are."""
    for filt in (os.path.join(LLVM, 'llvm-cxxfilt'), 'c++filt'):
        try:
            out = subprocess.run([filt], input='\n'.join(names).encode(), check=True, capture_output=True).stdout.decode()
            return dict(zip(names, out.splitlines()))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {name: name for name in names}


def main(parent_path, result_path):
    parent_objects, parent, parent_resources = library_symbols(parent_path)
    result_objects, result, result_resources = library_symbols(result_path)
    only_parent, only_result = sorted(set(parent) - set(result)), sorted(set(result) - set(parent))
    shared = sorted(set(parent) & set(result))
    differing = [name for name in shared if parent[name] != result[name]]
    names = demangled(only_parent + only_result + differing)
    print('| | parent | result |\n|---|---|---|')
    print('| code objects with gfx950 code | %d | %d |' % (parent_objects, result_objects))
    print('| kernel / device function symbols | %d | %d |' % (len(parent), len(result)))
    print('| only in one of the two | %d | %d |' % (len(only_parent), len(only_result)))
    print('| compared (size + instruction text) | %d | |' % len(shared))
    print('| differing | %d | |' % len(differing))
    for title, listed in (('only in the parent', only_parent), ('only in the result', only_result)):
        for name in listed:
            print('%s: %s' % (title, names[name]))
    if differing:
        print('\n| symbol | parent | result | parent resources | result resources |\n|---|---|---|---|---|')
    for name in differing:
        sizes = ['/'.join('%d B' % size for size, _ in side[name]) for side in (parent, result)]
        figures = [' '.join('%s=%s' % (key.strip('.'), value) for key, value in sorted(side.get(name, {}).items()))
                   for side in (parent_resources, result_resources)]
        print('| `%s` | %s | %s | %s | %s |' % (names[name], sizes[0], sizes[1], figures[0], figures[1]))
    changed = [name for name in shared if name in parent_resources and parent_resources[name] != result_resources.get(name)]
    print('\nkernels whose resource figures (%s) differ: %d' % (', '.join(RESOURCES), len(changed)))
    for name in changed:
        print('  %s: %s -> %s' % (demangled([name])[name], parent_resources[name], result_resources.get(name)))
    return 1 if (only_parent or only_result or differing or changed) else 0


if __name__ == '__main__':
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
