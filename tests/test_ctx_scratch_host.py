"""The validator context's scratch owner (pde-engine_amd/csrc/pdeval_scratch.h, pdeval_devbuf.h)
on the CPU under failing allocations: allocation failure is never provoked on a GPU, so the
rules the owner enforces -- capacity 0 after any failure, the hoist slots and their owner words
only together, the buffer epoch moving with every pointer -- are checked here."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SIM = os.path.join(HERE, 'hostsim')
GUARD = os.path.join(SIM, '_build', 'guard_ctx_scratch')
SRC = [os.path.join(ROOT, 'pde-engine_amd', 'csrc', f) for f in ('pdeval_scratch.h', 'pdeval_devbuf.h')] + \
      [os.path.join(SIM, 'guard_ctx_scratch.cpp')]


def test_scratch_owner_under_failing_allocations():
    """tests/hostsim/guard_ctx_scratch.cpp (its own main, stand-ins for the HIP calls the headers
    use) built with -fsanitize=address,undefined and run directly: reserve(1), reserve(1025),
    reserve(5000) for every hoist / hoist_slots / tier2_mask combination, every allocating call
    of each made to fail once."""
    if not os.path.exists(GUARD) or any(os.path.getmtime(s) > os.path.getmtime(GUARD) for s in SRC):
        os.makedirs(os.path.dirname(GUARD), exist_ok=True)
        subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-fsanitize=address,undefined',
                               '-fno-sanitize-recover=all', '-o', GUARD, SRC[-1]])
    r = subprocess.run([GUARD], capture_output=True, text=True)
    assert r.returncode == 0 and 'guard: 0 failures' in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
