"""fc_strip.hip and fc_strip16.hip name all 256 accumulator registers literally (the stationary strip).  hipcc must not have put
anything of its own there -- neither a parked value (v_accvgpr_* outside the asm statements) nor a spill -- and must not have gone to
scratch: compile each file with -save-temps and audit the ISA of its kernels (tools/debug/isa_audit.py)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# per file: its kernels, the MFMAs of one body (half a column block), its MFMA and the other shape's, which must not appear
@pytest.mark.parametrize('source,kernel,body_mfmas,mfma,other', [
    ('fc_strip16.hip', 'fc_strip16_kernel', 96, 'v_mfma_f32_16x16x32_f16', 'v_mfma_f32_32x32x16_f16'),
    ('fc_strip.hip', 'fc_strip_kernel', 48, 'v_mfma_f32_32x32x16_f16', 'v_mfma_f32_16x16x32_f16'),
], ids=['fc_strip16', 'fc_strip'])
def test_strip_kernels_keep_out_of_the_accumulator_registers(tmp_path, source, kernel, body_mfmas, mfma, other):
    from laff_amd import build
    sys.path.insert(0, os.path.join(ROOT, 'tools', 'debug'))
    import isa_audit
    src = os.path.join(build.CSRC, source)
    r = subprocess.run([build.hipcc()] + build.FLAGS + ['-save-temps=obj', '-c', src, '-o', str(tmp_path / source.replace('.hip', '.o'))],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    asm = [str(tmp_path / f) for f in os.listdir(tmp_path) if f.endswith('gfx950.s')]
    assert len(asm) == 1
    stats = isa_audit.audit(asm[0], kernel, quiet=True)
    assert len(stats) == 3                                    # the three epilogue kinds
    for name, st in stats.items():
        assert st['acc_outside'] == 0 and st['scratch'] == 0, (name, st)
        # the bodies instantiated per kernel: the plain loop's four + two tails of four
        assert st['mfma'] == 12 * body_mfmas, (name, st)
    text = open(asm[0]).read()
    assert mfma in text and other not in text
    for name in stats:
        meta = text[text.index('.name:           ' + name):]
        assert int(re.search(r'\.vgpr_spill_count: (\d+)', meta).group(1)) == 0
        assert int(re.search(r'\.sgpr_spill_count: (\d+)', meta).group(1)) == 0
