"""Every profile bench.py reads at run time was made on the kernels of the in-tree build
(VERDICT r4 next #7).

bench.py prices the level kernel's live time with an issue-cycle model and reads HBM traffic,
clock and profiled occupancy from committed PMC passes; it checks each file's recorded ISA hash
against the library it loaded and reports null fields on a mismatch.  This CPU test turns a
stale profile into a failing suite instead of a silent null on the driver's box: the hash of
each profiled kernel instance (tools/kernel_hash.py, from the gfx950 code objects inside
libdmstereo.so, instances derived from dm_build_config) must equal the hash the profile
recorded.  Runs wherever the library is built (the driver's build() step builds it here)."""
import json
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))
import kernel_hash as K  # noqa: E402

LIB = os.path.join(REPO, 'deepmatching_stereo_matching_amd', 'libdmstereo.so')
LEVEL = {128: 'pmc_level1.json', 64: 'pmc_level1_s64.json', 256: 'pmc_level1_s256.json'}
VOLUME = {(128, 4, False): 'pmc_volume.json', (128, 4, True): 'pmc_volume_mm.json',
          (128, 2, False): 'pmc_volume_f16.json', (128, 2, True): 'pmc_volume_f16_mm.json',
          (256, 4, False): 'pmc_volume_s256.json', (256, 4, True): 'pmc_volume_mm_s256.json',
          (256, 2, False): 'pmc_volume_f16_s256.json', (256, 2, True): 'pmc_volume_f16_mm_s256.json'}

_needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libdmstereo.so not built")


def _load(name):
    with open(os.path.join(REPO, 'profiles', name)) as f:
        return json.load(f)


@_needs_lib
@pytest.mark.parametrize('tile', sorted(LEVEL))
def test_level_profiles_match_build(tile):
    d = _load(LEVEL[tile])
    cur = K.kernel_hash(K.symbol('level', tile, lib=LIB), LIB)
    assert cur, 'profiled level-kernel instance not in the library'
    assert d.get('isa_sha16') == cur, '%s: PMC pass made on ISA %s, the build holds %s' % (
        LEVEL[tile], d.get('isa_sha16'), cur)
    assert d.get('issue_model_isa_sha16') == cur, '%s: issue model made on ISA %s, the build holds %s' % (
        LEVEL[tile], d.get('issue_model_isa_sha16'), cur)
    # the model's instruction count was checked against the PMC pass of the same build
    assert abs(d['issue_model_insts_vs_pmc'] - 1.0) < 0.03, d['issue_model_insts_vs_pmc']


@_needs_lib
@pytest.mark.parametrize('key', sorted(VOLUME))
def test_volume_profiles_match_build(key):
    d = _load(VOLUME[key])
    tile, esz, mm = key
    cur = K.kernel_hash(K.symbol('volume', tile, esz, mm, lib=LIB), LIB)
    assert cur, 'profiled volume-kernel instance not in the library'
    assert d.get('isa_sha16') == cur, '%s: PMC pass made on ISA %s, the build holds %s' % (
        VOLUME[key], d.get('isa_sha16'), cur)


@_needs_lib
def test_level_kernel_instances_are_exactly_the_launchable_ones():
    """The library holds the k_level1_mfq / k_level12_* instances the dispatch can launch and no
    other (level_kernel / launch_level in dm_kernels.hip), each for dm_corr_level1 (L2F = 0) and
    dm_corr_level12 (L2F = 1):
      ws >= 7            k_level1_mfq<KS, 2, NW, 5, L2F, false>: KS = ceil(ws^2 / 64) = 1 .. 4,
                         NW = w0 / 32 = 1, 2, 4, 8 (w0 = 32, 64, 128, 256)
      ws <= 5, w0 = 32   k_level1_mfq<1, 2, 1, 5, L2F, true>: the packed-f32 y (YF); the wider
                         ws <= 5 shapes all have strips
      ws <= 5, w0 = 128  k_level1_mfq<1, 4, 2 C3_NB, C3_MINW, L2F, true, C3_NB, F16 = true>
      ws <= 5, w0 = 64   k_level12_strip<1, C2_NB, L2F>;  w0 = 256: k_level12_strip<4, C5_NB, L2F>
    A dead instance that comes back (a launch behind a run-time `if` over compile-time constants
    still instantiates its kernel), or the pruned kernel, fails here."""
    c = dict(K.DEFAULTS, **K.build_config(LIB))
    mfq = '_Z12k_level1_mfqILi%dELi%dELi%dELi%dELb%dELb%dELi%dELb%dEE'
    want = {mfq % (ks, 2, nw, 5, l2f, yf, 1, 0)
            for ks in (1, 2, 3, 4) for nw in (1, 2, 4, 8) for l2f in (0, 1) for yf in (0, 1)
            if not yf or (ks, nw) == (1, 1)}
    want |= {mfq % (1, 4, 2 * c['C3_NB'], c['C3_MINW'], l2f, 1, c['C3_NB'], 1) for l2f in (0, 1)}
    want |= {'_Z15k_level12_stripILi%dELi%dELb%dEE' % (nwc, c[nb], l2f)
             for nwc, nb in ((1, 'C2_NB'), (4, 'C5_NB')) for l2f in (0, 1)}
    assert len(want) == 40
    data = open(LIB, 'rb').read()
    have = set()
    for base in K._elfs(data):
        syms = K._symbols(data, base)
        have |= {nm[:nm.index('v3Geo')] for nm in syms
                 if nm + '.kd' in syms and ('k_level1_mfq' in nm or 'k_level12_' in nm)}
    assert not any('k_level12_prune' in nm for nm in have)
    assert have == want, (sorted(have - want), sorted(want - have))


def test_hash_masks_pc_relative_table_offsets():
    """The ISA hash ignores the literals of s_getpc_b64 + s_add_u32 / s_addc_u32 (the constant
    tables' PC-relative offsets, which move when another kernel grows) and nothing else."""
    import struct
    getpc, add, addc = 0xBE861C00, 0x8006FF06, 0x8207FF07   # s_getpc_b64 s[6:7]; s_add(c)_u32 s6/s7, lit
    other = 0xD2080002
    a = struct.pack('<7I', getpc, add, 0xFFF62910, addc, 0xFFFFFFFF, other, 0x12345678)
    b = struct.pack('<7I', getpc, add, 0x00001234, addc, 0x00000000, other, 0x12345678)
    c = struct.pack('<7I', getpc, add, 0x00001234, addc, 0x00000000, other, 0x12345679)
    assert K._mask_pc_literals(a) == K._mask_pc_literals(b)
    assert K._mask_pc_literals(b) != K._mask_pc_literals(c)
    # a literal after an add that does not follow s_getpc stays part of the hash
    d = struct.pack('<3I', add, 0x1, other)
    e = struct.pack('<3I', add, 0x2, other)
    assert K._mask_pc_literals(d) != K._mask_pc_literals(e)


def _profiles_with_symbols():
    import glob
    out = []
    for f in sorted(glob.glob(os.path.join(REPO, 'profiles', '*.json'))):
        try:
            d = json.load(open(f))
        except ValueError:
            continue

        def walk(x, path):
            if isinstance(x, dict):
                if isinstance(x.get('kernel'), str) and x.get('isa_symbol'):
                    out.append((path, x['kernel'], x['isa_symbol']))
                for k, v in x.items():
                    walk(v, path + '/' + k)
        walk(d, os.path.basename(f))
    return out


@pytest.mark.parametrize('path,label,sym', _profiles_with_symbols())
def test_profile_label_names_the_profiled_kernel(path, label, sym):
    """A profile's "kernel" label is the kernel its isa_symbol names (the
    strip kernel's passes were labelled k_level1_mfq)."""
    assert label.split(' ')[0] == sym.split('I', 1)[0], (path, label, sym)


def _vregs(tok):
    """VGPR numbers named by one operand token ('v7', 'v[2:3]'), else ()."""
    import re
    m = re.match(r'^v(\d+)$', tok) or re.match(r'^v\[(\d+):(\d+)\]$', tok)
    if not m:
        return ()
    lo = int(m.group(1))
    hi = int(m.group(2)) if m.lastindex == 2 else lo
    return tuple(range(lo, hi + 1))


def dpp_hazards(disasm_lines):
    """(function, line) of every DPP instruction whose DPP source VGPR was written by a VALU
    instruction within the 2 wait states before it (gfx9: VALU write VGPR -> DPP read of it needs
    2; s_nop n supplies n + 1), scanning each function's instructions in order."""
    import re
    bad, fn, recent = [], None, []   # recent: the written-VGPR sets of the last wait-state slots
    for ln in disasm_lines:
        if re.match(r'^[0-9a-f]+ <.*>:$', ln.strip()):
            fn, recent = ln.strip(), []
            continue
        s = ln.split('//')[0].strip()
        if not s or s.endswith(':'):
            continue
        op, _, rest = s.partition(' ')
        ops = [t.strip() for t in rest.split(',')] if rest else []
        if '_dpp' in op and len(ops) >= 2:
            src = set(_vregs(ops[1].split()[0]))
            if any(src & w for w in recent[-2:]):
                bad.append((fn, s))
        if op == 's_nop':
            recent.extend([set()] * (int(ops[0], 0) + 1) if ops else [set()])
        elif op.startswith('v_') and not op.startswith(('v_cmp', 'v_readlane', 'v_readfirstlane')) and ops:
            recent.append(set(_vregs(ops[0])))
        else:
            recent.append(set())
        recent = recent[-2:]
    return bad


def test_dpp_hazard_checker_itself():
    ok = ['0000 <k>:', 'v_add_f32_e32 v5, v1, v2', 's_nop 1',
          'v_min_f32_dpp v5, v5, v5 row_ror:8 row_mask:0xf bank_mask:0xf']
    bad = ['0000 <k>:', 'v_add_f32_e32 v5, v1, v2', 'v_mov_b32_e32 v6, v1',
           'v_min_f32_dpp v5, v5, v5 row_ror:8 row_mask:0xf bank_mask:0xf']
    wide = ['0000 <k>:', 'v_pk_mul_f32 v[4:5], v[0:1], v[2:3]', 's_nop 0',
            'v_max_f32_dpp v5, v5, v5 row_ror:8 row_mask:0xf bank_mask:0xf']
    assert dpp_hazards(ok) == [] and len(dpp_hazards(bad)) == 1 and len(dpp_hazards(wide)) == 1


@_needs_lib
def test_no_dpp_read_after_valu_write_hazard_in_library(tmp_path):
    """half_wave_minmax issues DPP min/max from inline asm, which the compiler's hazard
    recognizer cannot see; its s_nop and the instruction order inside the sequence are what keep
    a DPP read >= 2 wait states after the VALU write of its operand.  The check runs over the
    built gfx950 code, every kernel, so a register copy the compiler places in between fails it."""
    import shutil
    import struct
    import subprocess
    objdump = '/opt/rocm/lib/llvm/bin/llvm-objdump'
    if not os.path.exists(objdump):
        pytest.skip('llvm-objdump not available')
    data = open(LIB, 'rb').read()
    n_dpp = 0
    for i, base in enumerate(K._elfs(data)):
        shoff, = struct.unpack_from('<Q', data, base + 0x28)
        shentsize, shnum = struct.unpack_from('<HH', data, base + 0x3A)
        co = tmp_path / ('co%d.elf' % i)
        co.write_bytes(data[base:base + shoff + shnum * shentsize])
        out = subprocess.run([objdump, '-d', '--no-show-raw-insn', str(co)], capture_output=True,
                             text=True, check=True).stdout.splitlines()
        n_dpp += sum('_dpp' in ln for ln in out)
        bad = dpp_hazards(out)
        assert not bad, bad[:5]
    assert n_dpp > 0
