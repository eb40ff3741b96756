"""fc_strip16.hip names all 256 accumulator registers literally (the stationary strip), as fc_strip.hip does.  hipcc must not have put
anything of its own there -- neither a parked value (v_accvgpr_* outside the asm statements) nor a spill -- and must not have gone to
scratch: compile the file with -save-temps and audit the ISA of its kernels (tools/debug/isa_audit.py)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fc_strip16_kernels_keep_out_of_the_accumulator_registers(tmp_path):
    from laff_amd import build
    sys.path.insert(0, os.path.join(ROOT, 'tools', 'debug'))
    import isa_audit
    src = os.path.join(build.CSRC, 'fc_strip16.hip')
    r = subprocess.run([build.hipcc()] + build.FLAGS + ['-save-temps=obj', '-c', src, '-o', str(tmp_path / 'fc_strip16.o')],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    asm = [str(tmp_path / f) for f in os.listdir(tmp_path) if f.endswith('gfx950.s')]
    assert len(asm) == 1
    stats = isa_audit.audit(asm[0], 'fc_strip16_kernel', quiet=True)
    assert len(stats) == 3                                    # the three epilogue kinds
    for name, st in stats.items():
        assert st['acc_outside'] == 0 and st['scratch'] == 0, (name, st)
        # the bodies instantiated per kernel: the plain loop's four + two tails of four (fc_strip16.hip), 96 MFMAs 16x16x32 each
        assert st['mfma'] == 12 * 96, (name, st)
    text = open(asm[0]).read()
    assert 'v_mfma_f32_32x32x16_f16' not in text
    for name in stats:
        meta = text[text.index('.name:           ' + name):]
        assert int(re.search(r'\.vgpr_spill_count: (\d+)', meta).group(1)) == 0
        assert int(re.search(r'\.sgpr_spill_count: (\d+)', meta).group(1)) == 0
