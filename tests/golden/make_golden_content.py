"""Reference fixtures of the content classes (synthetic.content_pair) at an MFMA shape, S = 32.

Run in the build container only, like make_golden.py, whose run_pair / save this imports: the
reference modules run unchanged on the repo's pinned matchTemplate, and only inputs and outputs
are written (npz data), never reference source.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_content.py

The S = 16 fixtures with ties / noise / NaN maps (pair_s16_ws5_*) never reach the MFMA, fused
or on-demand kernels; these do: `dark` (flat patches: NaN maps next to textured ones),
`checker` (every level-0 row has many exact maxima), `edge` (nearly all patches flat, the rest
at every extreme) with TM_CCOEFF_NORMED, `binary` with TM_CCOEFF.  Sampled form (full_levels=
False), as pair_s32_ws5.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from make_golden import run_pair, save  # noqa: E402

from deepmatching_stereo_matching_amd.synthetic import content_pair  # noqa: E402


def main():
    for kind in ('dark', 'checker', 'edge'):
        a, b = content_pair(kind, 36, 36, 11)
        save('pair_s32_ws5_' + kind, run_pair(a, b, 5, 'normed', False))
    a, b = content_pair('binary', 36, 36, 11)
    save('pair_s32_ws5_binary_ccoeff', run_pair(a, b, 5, 'ccoeff', False))


if __name__ == '__main__':
    main()
