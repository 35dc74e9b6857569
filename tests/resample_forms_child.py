"""Child process of tests/test_gpu_resample.py::test_register_and_lds_forms_agree_in_the_tuning_build: with SOUNDSCOPE_HIP_LIB naming a
-DSS_TUNING build of the library and SS_RESAMPLE_FORM naming a kernel form, converts the seeded streams of every case and leaves each
case's outputs and tile plan in <out_dir>/<in>_<out>_<channels>.npz.  No test of its own."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [(44100, 48000, 1), (44100, 48000, 2), (48000, 44100, 1), (48000, 44100, 2)]
# around the tile edges of both forms (3822 / 3969 and 3840 / 4000 input frames in stereo), and the ends
LENGTHS = [0, 1, 37, 147, 160, 3821, 3822, 3823, 3839, 3840, 3841, 3968, 3969, 3970, 3999, 4000, 4001, 8071]


def streams_of(case):
    rng = np.random.default_rng(case[0] + case[2])
    return [(0.3 * rng.standard_normal((F, case[2]))).astype(np.float32) for F in LENGTHS]


def main(out_dir):
    import soundscope_amd as ssa
    from soundscope_amd import _lib as L
    from soundscope_amd.batch import resample_plan
    for case in CASES:
        in_rate, out_rate, ch = case
        plan = resample_plan(in_rate, out_rate)
        xs = streams_of(case)
        fps = max(LENGTHS) | 1
        slab = np.full((len(xs), fps, ch), 0.5, np.float32)
        for s, x in enumerate(xs):
            slab[s, :x.shape[0]] = x
        src = ssa.Batch(in_rate, ch, len(xs), fps, flags=L.SS_BATCH_TRUE_PEAK)
        src.upload(0, slab)
        src.set_lengths(LENGTHS)
        tiles = src.resample_tiles(plan)
        dst = src.resample(out_rate)
        outs = {"s%d" % s: dst.download_input(s)[:int(dst.stream_shape(s).frames) * ch] for s in range(len(xs))}
        np.savez(os.path.join(out_dir, "%d_%d_%d.npz" % case), tiles=np.asarray(tiles), **outs)
        src.close()
        dst.close()


if __name__ == "__main__":
    main(sys.argv[1])
