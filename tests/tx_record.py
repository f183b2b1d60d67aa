"""How profiles/tx_parity.txt is made -- TEST INFRASTRUCTURE, apart from the reference model (tx_model.py).

With TX_PARITY_OUT=<file> set, every comparison of test_tx_model_cpu.py ("oracle" lines) and test_gpu_tx.py ("gpu" lines) appends
one line to <file>; unset, nothing is written.  The helper only ever APPENDS: remove <file> before regenerating, run the CPU module
and then the GPU module once each, and put the header of profiles/tx_parity.txt in front."""
import os

import noise_model as NM
import tx_model as T


def record(side, case, res, bits):
    """one line per comparison with the model: the share off rint(v) and the largest distance of such a sample's v from its rounding
    boundary, in units of full scale, in LSB of the comparison's own width and as a fraction of the tolerance"""
    path = os.environ.get("TX_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write("%-6s %-62s n %8d  differ %6d  share %8.5f %%  unexplained %d  worst %9.3e fs = %7.5f LSB%-2d = %5.3f tol\n" % (
                side, case, res.n, res.n - res.equal, 100.0 * NM.share(res), res.unexplained, res.worst * T.TOL_FS,
                res.worst * T.tol_lsb(bits), bits, res.worst))
