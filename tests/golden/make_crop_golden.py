"""Fixtures for the crop-and-resize front end from the reference's OWN transform class.

    python tests/golden/make_crop_golden.py <path to a checkout of the reference>    ->  tests/golden/crop_reference.npz

deephar/utils/transform.py of the reference is loaded at run time (nothing of it is copied here) and its class T is driven
the way the loaders drive it in test mode (deephar/data/mpii.py:114-121, pennaction.py:157-163):
    T(Image).rotate_crop(0, objpos, winsize); .resize(crop_resolution); [.horizontal_flip()]; .normalize_affinemap(); .asarray()
on seeded synthetic images (tests/cropref.synthetic_image).  Stored per case: seed, image shape, objpos, winsize, output size,
hflip and the OUTPUTS only -- the uint8 crop, the integer box, afmat -- plus the Pillow version that produced them.  The
reference pins Pillow 5.1.0; these were made with the Pillow of the machine that ran this script."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cropref  # noqa: E402

OUT = os.path.join(HERE, 'crop_reference.npz')

# (seed, H, W, objpos, winsize, (OW, OH), hflip)
CASES = [
    (1, 60, 80, (10.0, 12.0), (50.0, 50.0), (32, 32), 0),        # a negative corner
    (2, 60, 80, (70.0, 50.0), (44.0, 44.0), (32, 32), 1),        # beyond the right and bottom edges, mirrored
    (3, 90, 70, (10.3, 30.6), (50.0, 50.0), (24, 32), 0),        # a square window truncated toward zero to 49 x 50: (-14, 5, 35, 55)
    (4, 90, 70, (10.3, 30.6), (50.0, 50.0), (24, 32), 1),
    (5, 20, 24, (12.0, 10.0), (14.0, 12.0), (64, 48), 0),        # up-scaling
    (6, 20, 24, (12.5, 9.5), (9.0, 7.0), (48, 40), 1),           # up-scaling, odd window, mirrored
    (7, 200, 260, (130.0, 100.0), (150.0, 150.0), (32, 32), 0),  # down-scaling by 4.6875
    (8, 200, 260, (128.7, 97.2), (171.0, 163.0), (32, 24), 1),   # down-scaling by 5.3 / 6.8, non-square
    (9, 64, 64, (32.0, 32.0), (64.0, 64.0), (64, 48), 0),        # cw == OW: the horizontal pass is the identity
    (10, 50, 50, (-10.0, 25.0), (40.0, 40.0), (16, 16), 0),      # mostly outside on the left
    (11, 48, 64, (32.0, 24.0), (100.0, 90.0), (40, 36), 1),      # the window contains the whole image
    (12, 33, 47, (23.5, 16.5), (47.0, 33.0), (47, 33), 0),       # the whole image at its own size: identity in both passes
]


def load_transform(ref_root):
    path = os.path.join(ref_root, 'deephar', 'utils', 'transform.py')
    spec = importlib.util.spec_from_file_location('reference_transform', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('DEEPHAR_REFERENCE')
    if not ref_root:
        raise SystemExit(__doc__)
    import PIL
    from PIL import Image
    tr = load_transform(ref_root)
    out = {'pillow_version': np.array(PIL.__version__), 'num_cases': np.array(len(CASES))}
    for i, (seed, H, W, objpos, winsize, size, hflip) in enumerate(CASES):
        img = cropref.synthetic_image(seed, H, W)
        t = tr.T(Image.fromarray(img))
        t.rotate_crop(0, np.array(objpos), winsize)
        box = np.array([-t.afmat[0, 2], -t.afmat[1, 2]])              # what crop() translated by: the integer corner
        cw, ch = t.size
        t.resize(size)
        if hflip:
            t.horizontal_flip()
        t.normalize_affinemap()
        frame = t.asarray(dtype=np.uint8)
        assert frame.shape == (size[1], size[0], 3)
        out.update({'seed_%d' % i: np.array(seed), 'shape_%d' % i: np.array([H, W]), 'objpos_%d' % i: np.array(objpos),
                    'winsize_%d' % i: np.array(winsize), 'size_%d' % i: np.array(size), 'hflip_%d' % i: np.array(hflip),
                    'frame_%d' % i: frame, 'afmat_%d' % i: t.afmat.copy(),
                    'box_%d' % i: np.array([box[0], box[1], box[0] + cw, box[1] + ch]).astype(np.int64)})
    np.savez_compressed(OUT, **out)
    print('wrote %s (%d cases, Pillow %s, %d bytes)' % (OUT, len(CASES), PIL.__version__, os.path.getsize(OUT)))


if __name__ == '__main__':
    main()
