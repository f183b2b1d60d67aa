"""How profiles/demod_parity.txt is made -- TEST INFRASTRUCTURE, apart from the reference model (demod_model.py).

With DEMOD_PARITY_OUT=<file> set, every comparison of test_demod_model_cpu.py ("oracle" lines) and test_gpu_demod.py ("gpu" lines)
appends one line to <file>; unset, nothing is written.  The helper only ever APPENDS: remove <file> before regenerating, run the CPU
module and then the GPU module once each, and put the header of profiles/demod_parity.txt in front."""
import os


def record(side, case, verdict, tol):
    """one line per comparison with the model: worst and median d, the worst absolute distance, erasure ties, unexplained points and
    the T in force"""
    path = os.environ.get("DEMOD_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write("%-6s %-58s n %6d  worst %6.3f  median %5.3f  abs %9.3e  ties %3d  unexplained %d  T %5.2f\n" % (
                side, case, verdict.n, verdict.worst, verdict.median, verdict.worst_abs, verdict.ties, verdict.unexplained, tol))
