"""Writes tests/golden/conv_routes.json: what every convolution / GEMM call of tests/conv_route_cases.py launches on the
MI355X, as the library's own profile report states it.  Uses the public ABI only, so it runs unchanged on any commit:

    python tests/golden/make_conv_route_goldens.py [OUT.json]

Record at the commit BEFORE a change to the host-side routing; test_conv_routes_gpu.py then holds the change to it."""
import json
import os
import sys

GOLDEN = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(GOLDEN))                    # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(GOLDEN)))   # the repository root


def write(routes, path):
    """One line per case: the file stays readable in a diff."""
    with open(path, 'w') as handle:
        handle.write('{\n')
        for g, group in enumerate(sorted(routes)):
            handle.write(f' {json.dumps(group)}: {{\n')
            cases = sorted(routes[group])
            for i, case in enumerate(cases):
                body = json.dumps(routes[group][case], sort_keys=True, separators=(',', ':'))
                handle.write(f'  {json.dumps(case)}: {body}{"," if i + 1 < len(cases) else ""}\n')
            handle.write(' }' + (',' if g + 1 < len(routes) else '') + '\n')
        handle.write('}\n')


def main():
    import srgan_amd  # noqa: F401
    from srgan_amd import _lib
    import conv_route_cases
    routes, _ = conv_route_cases.replay(_lib.library())
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(GOLDEN, 'conv_routes.json')
    write(routes, path)
    calls = sum(len(case) for group in routes.values() for case in group.values())
    print(f'{path}: {calls} calls, {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
