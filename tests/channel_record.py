"""How profiles/channel_parity.txt is made -- TEST INFRASTRUCTURE, apart from the reference model (noise_model.py).

With CHANNEL_PARITY_OUT=<file> set, every comparison of test_noise_model_cpu.py ("oracle" lines) and test_gpu_channel.py ("gpu"
lines) appends one line to <file>; unset, nothing is written.  The helper only ever APPENDS: remove <file> before regenerating,
run the CPU module and then the GPU module once each, and put the header of profiles/channel_parity.txt in front."""
import os

import noise_model as NM


def record(side, case, res):
    """one line per comparison: the differing share and the largest distance to a rounding boundary as a fraction of the tolerance"""
    path = os.environ.get("CHANNEL_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write("%-6s %-58s n %8d  differ %6d  share %8.5f %%  unexplained %d  worst %5.3f tol\n" % (
                side, case, res.n, res.n - res.equal, 100.0 * NM.share(res), res.unexplained, res.worst))
