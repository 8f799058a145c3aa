"""SpecAugment as the reference's loader applies it (``augmentation.spec_augment: True`` -> ``spec_augment(spect)``,
loader/spec_augment.py:68-115, called per clip after normalisation, loader/data_loader.py:162-163): the random DRAWS are made here
on the host, everything that touches the spectrogram runs on the device (csrc/ds2_spect.hip).

The reference's time warp is not the paper's: ``time_warp`` (:48-65, always its default W = 5 -- ``time_warping_para`` is never
passed on) picks a frame i, reads the spectrogram VALUE pt = spec[F//2][i] and uses it as a time coordinate of the single control
point (F//2, pt) -> (F//2, pt + d) of ``sparse_image_warp``.  The resulting flow is affine in (f, t), zero along frequency, and
depends on the 3 x 3 block of ``randn / 1e10`` that loader/sparse_image_warp.py:170 puts into the otherwise singular system; so
that block is part of the draw.  This is what models trained with the reference's configurations have seen, and what is
reproduced.

Deviation: a clip with T <= 2W frames (0.1 s) makes the reference's ``randrange(W, T - W)`` raise ValueError; here it is left
unwarped (masks still apply)."""
import numpy as np

MAX_MASKS = 4           # masks per axis and clip that the kernels take


class SpecAugment:
    def __init__(self, frequency_masking_para=27, time_masking_para=70, frequency_mask_num=1, time_mask_num=1, W=5):
        self.frequency_masking_para, self.time_masking_para = frequency_masking_para, time_masking_para
        self.frequency_mask_num, self.time_mask_num, self.W = int(frequency_mask_num), int(time_mask_num), int(W)
        self._check()

    def _check(self):
        if not (0 <= self.frequency_mask_num <= MAX_MASKS and 0 <= self.time_mask_num <= MAX_MASKS):
            raise ValueError("the device kernels take up to %d frequency and %d time masks per clip; got %d / %d"
                             % (MAX_MASKS, MAX_MASKS, self.frequency_mask_num, self.time_mask_num))
        if self.W < 1:
            raise ValueError("W must be positive")

    def _masks(self, rng, num, para, size):
        m = np.zeros((num, 2), np.int32)
        for k in range(num):
            w = int(rng.uniform(0.0, para))                 # spec_augment.py:99-100 / :108-109
            if size - w < 0:                                # :101 / :110: a mask wider than the axis is skipped
                continue
            m[k] = int(rng.integers(0, size - w, endpoint=True)), w      # random.randint: both ends inclusive
        return m

    def draw(self, frames, n_bins, rng):
        """One set of draws per clip from a numpy.random.Generator, in the reference's order (warp, frequency masks, time masks).
        frames: the clips' frame counts.  Returns (warp_draw [N][12] float32: i, d, the nine values of randn(3, 3) / 1e10, 0;
        fmask [N][MF][2] int32, tmask [N][MT][2] int32: start and width, width 0 = no mask)."""
        self._check()
        frames = np.asarray(frames, np.int64).reshape(-1)
        N, W = len(frames), self.W
        warp = np.zeros((N, 12), np.float32)
        fmask = np.zeros((N, self.frequency_mask_num, 2), np.int32)
        tmask = np.zeros((N, self.time_mask_num, 2), np.int32)
        for n, T in enumerate(frames):
            T = int(T)
            if T > 2 * W:
                warp[n, 0] = rng.integers(W, T - W)         # random.randrange(W, T - W): upper end exclusive (:56)
                warp[n, 1] = rng.integers(-W, W)            # random.randrange(-W, W) (:60)
                warp[n, 2:11] = rng.standard_normal(9) / 1e10
            else:
                warp[n, 0] = -1
            fmask[n] = self._masks(rng, self.frequency_mask_num, self.frequency_masking_para, int(n_bins))
            tmask[n] = self._masks(rng, self.time_mask_num, self.time_masking_para, T)
        return warp, fmask, tmask
