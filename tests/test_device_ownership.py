"""Device memory, pinned memory, events and streams have ONE owner each (rust-doom_amd/csrc/hip/device_memory.hpp): no other source
file calls the runtime's allocate / create / release functions, so a handle's destroy function is `delete` and a local is released
on every way out of its function.  A feature that needs a buffer declares a DeviceArray."""
import glob
import os
import re

from util import ROOT

CSRC = os.path.join(ROOT, 'rust-doom_amd', 'csrc')
OWNERS = os.path.join(CSRC, 'hip', 'device_memory.hpp')
CALLS = re.compile(r'hipMalloc\(|hipFree\(|hipHostMalloc\(|hipHostFree\(|hipEventCreate|hipEventDestroy|hipStreamCreate|hipStreamDestroy')


def _sources():
    return [p for ext in ('hip', 'hpp', 'cpp', 'h') for p in glob.glob(os.path.join(CSRC, '**', '*.' + ext), recursive=True)]


def test_only_the_owners_call_the_runtimes_allocators():
    assert OWNERS in _sources()
    found = [(os.path.relpath(p, ROOT), n) for p in _sources() if p != OWNERS
             for n, line in enumerate(open(p, encoding='utf-8'), 1) if CALLS.search(line)]
    assert not found, found
    assert len(set(CALLS.findall(open(OWNERS, encoding='utf-8').read()))) == 8  # each of them is there, once per kind


def test_every_destroy_function_is_delete():
    bodies = {}
    for p in _sources():
        for m in re.finditer(r'^void (rdoom_\w+_destroy)\(\w+ \*(\w+)\) \{(.*?)\}\n', open(p, encoding='utf-8').read(), re.M | re.S):
            bodies[m.group(1)] = (m.group(2), m.group(3).strip())
    assert {'rdoom_level_destroy', 'rdoom_batch_destroy', 'rdoom_world_destroy', 'rdoom_worldset_destroy', 'rdoom_lightset_destroy',
            'rdoom_thingset_destroy'} <= set(bodies), sorted(bodies)
    for name, (arg, body) in bodies.items():
        assert body == 'delete %s;' % arg, (name, body)  # (delete takes a null pointer)
