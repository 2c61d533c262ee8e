"""
Record tests/golden/gless_probes_parent.npz: negf_gless_int_probes at the automatic batch (one sweep over the grid) on
dephase_ref's shapes (a), (b) and (d), 70 energies, contact 0, contact 1 and the total, with the probes floating and
without probes -- the cases of tests/test_batch_cut_gpu.py::test_gless_int_probes_keeps_its_bits_under_every_cut.  The
record is that test's yardstick (bit for bit), so it is taken ONCE, on the GPU, from a build of the commit BEFORE the
weighted sum of negf_gless_int_probes got its grid chunks and carry:

    NEGF_LIB_PATH=/path/to/parent/libnegf_hip.so python scripts/gen_gless_probes_parent_fixture.py [out.npz]

Shapes (a) and (b) are kept in full; of shape (d)'s 130 x 130 sums the rows ROWS_D and a SHA-256 digest of all of them.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_batch_cut_gpu as bc  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else bc.GOLDEN
    from gaunegf_amd import _lib
    from gaunegf_amd.engine import get_engine
    print("library:", _lib.LIB_PATH)
    eng = get_engine()
    eng.set_batch(0)
    rec = {}
    for shape in bc.PROMISED:
        h, probes, E, w, free = bc.promised_system(eng, shape)
        try:
            sums = bc.promised_sums(eng, h, probes, E, w)
            assert eng.get_batch() >= E.size, (eng.get_batch(), E.size)        # one sweep
        finally:
            free()
        for tag, a in sums.items():
            key = f"{shape} {tag}"
            assert np.all(np.isfinite(a.view(np.float64))), key
            if shape == "d":
                rec[key + " sha256"] = np.array(bc.digest(a))
                rec[key + " rows"] = a[list(bc.ROWS_D)]
            else:
                rec[key] = a
            print(key, a.shape, bc.digest(a)[:16])
    np.savez(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
