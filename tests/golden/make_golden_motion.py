"""Golden vectors for the motion reader of the animation path, from the REAL `engineer.utils.snug_utils.load_motion`:

  motion_in.npz    a small synthetic AMASS / CMU style motion: 48 frames at 120 fps, `poses` [48,156] float64 (smooth random
                   rotations; only the first 72 columns are read), `trans` [48,3], `mocap_framerate`
  motion_out.npz   what the reference returns for it: pose [12,72], trans [12,3], trans_vel [12,3] (float32)

    python tests/golden/make_golden_motion.py
"""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.insert(0, str(HERE))
sys.path[:0] = [str(REPO / "rec-mv_amd"), str(REPO)]
import scipy.spatial.transform  # noqa: E402,F401  (the real scipy, before the loader's dummy finder is installed)
import ref_loader  # noqa: E402
from make_golden import save  # noqa: E402


def synthetic_motion(frames=48, rate=120.0, seed=21):
    rng = np.random.RandomState(seed)
    poses = 0.4 * rng.randn(1, 156) + np.cumsum(0.03 * rng.randn(frames, 156), axis=0)
    poses[:, :3] += np.array([1.2, -0.4, 0.7])                  # a root rotation well away from the identity
    trans = np.cumsum(0.01 * rng.randn(frames, 3), axis=0) + np.array([0.3, -0.2, 0.9])
    return {'poses': poses, 'trans': trans, 'mocap_framerate': np.float64(rate)}


def main():
    motion = synthetic_motion()
    np.savez(HERE / "motion_in.npz", **motion)
    snug = ref_loader.ref_module("engineer.utils.snug_utils")
    pose, trans, vel = snug.load_motion(str(HERE / "motion_in.npz"))
    save("motion_out", pose=pose, trans=trans, trans_vel=vel)


if __name__ == "__main__":
    main()
