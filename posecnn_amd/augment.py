"""The random draws of the reference's training augmentation — `chromatic_transform` and `add_noise`,
lib/utils/blob.py:74-129, called per frame by lib/gt_synthesize_layer/minibatch.py:170-201 — as the parameter rows of
`ops.augment_frames` (include/posecnn_hip_augment.h). The distribution, not the reference's random stream: the draws are
made on a seeded numpy Generator in the reference's order, with its ranges and probabilities; the per-pixel normal
deviates are drawn on the device from (seed, stream id, pixel), and every frame gets a stream id of its own, so a frame's
noise does not depend on its position in a batch.

    sampler = AugmentSampler(seed=0)                      cfg.TRAIN.CHROMATIC, cfg.TRAIN.ADD_NOISE
    data, data_p = ops.augment_frames(batch.color, batch.depth, sampler.sample(B), sampler.seed)
    feed = batch.feed(extents, points, symmetry, rgbd=True, augment=sampler)
"""
import numpy as np

ROW = 10                                     # PCNN_AUGMENT_ROW
MODE_NONE, MODE_GAUSS, MODE_HBLUR, MODE_VBLUR = 0, 1, 2, 3
BLUR_SIZES = (3, 5, 7, 9, 11, 15)            # blob.py:119


class AugmentSampler:
    """`sample(n)` -> float64 [n,10], one row per frame: (d_h, d_l, d_s, colour mode, sigma | size, colour stream id,
    chromatic, depth mode, sigma | size, depth stream id). `seed` (an integer below 2^128) seeds the Generator and is the
    Philox key `ops.augment_frames` takes. chromatic / add_noise: cfg.TRAIN.CHROMATIC / cfg.TRAIN.ADD_NOISE."""

    def __init__(self, seed=0, chromatic=True, add_noise=True):
        self.seed = int(seed)
        if not 0 <= self.seed < 1 << 128:
            raise ValueError("AugmentSampler: seed must be in [0, 2^128)")
        self.chromatic, self.add_noise = bool(chromatic), bool(add_noise)
        self.rng = np.random.default_rng(self.seed)
        self.next_stream = 0

    def _noise(self):
        """add_noise's draws (blob.py:105-125) -> (mode, sigma | size, a fresh stream id)"""
        rng = self.rng
        stream = self.next_stream
        self.next_stream += 1
        if not self.add_noise:
            return MODE_NONE, 0.0, stream
        if rng.random() < 0.9:
            var = rng.random() * 0.3 * 256
            return MODE_GAUSS, float(np.float32(np.sqrt(var))), stream
        size = BLUR_SIZES[int(rng.integers(len(BLUR_SIZES)))]
        return (MODE_HBLUR if rng.random() < 0.5 else MODE_VBLUR), float(size), stream

    def sample(self, n=1):
        rows = np.zeros((int(n), ROW), dtype=np.float64)
        for row in rows:
            if self.chromatic:                                   # blob.py:79-84
                row[0] = (self.rng.random() - 0.5) * 0.02 * 180
                row[1] = (self.rng.random() - 0.5) * 0.2 * 256
                row[2] = (self.rng.random() - 0.5) * 0.2 * 256
                row[6] = 1.0
            row[3:6] = self._noise()                             # minibatch.py:174-175
            row[7:10] = self._noise()                            # minibatch.py:192-193: the depth plane's own draws
        return rows
