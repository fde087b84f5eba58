"""Coverage contract: every kernel instantiation libtsff.so ships is reached by a case of CASES and compared there with a
high-precision reference.

CASES rows: (deck, B, entry point, launch plan, kernels the call must launch).  The deck is a dict of tweaks to
decks.deck_fit: n_ion, ppp (points per pixel), nvx, G (gradient points), m (DLM order trainable), fe (free-form f_e,
fe_mode PER_LINEOUT), sde / sdi (IRF widths), nang (scattering angles), z (every species' Z trainable), tie (ion-3's Ti tied to
ion-1's).  The launch planner (launch_spectrum in
tsff_api.inc) picks a form from the ion count, G, points per pixel, the LDS budget (nvx, npts, IRF taps), n_angles <= 16,
the batch against the CU count and the plan bits; tsff_last_launch reports what it picked.

Entry points: fwd (tsff_forward), lg (tsff_loss_grad), lgfe (tsff_loss_grad_fe), al (tsff_array_loss), chi
(tsff_chi_table), ff / ffg / ffg_fe (tsff_form_factor, its adjoint without / with the f_e adjoint), ff2d_fwd / ff2d_save /
ff2d_adj (the 2-D path; _lds: nv = 48, table in LDS; _l2: nv = 132, table read through L1/L2).

test_every_instantiation_has_a_case (CPU) fails when the library holds an instantiation of the listed families that no
case names, or a case names a kernel the library does not hold.  test_case_matches_reference (GPU) runs each case, checks
that it launched the kernels it names, and compares every output with the oracle at the suite's bounds.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import decks
import util
from oracle import tsadar_oracle as orc

# families under the contract (the other kernels take no template arguments or are measurement kernels)
FAMILIES = ("k_spectrum", "k_spectrum_fused", "k_spectrum_rows", "k_forward_pairs", "k_form_factor", "k_form_factor_adj",
            "k_form_factor_2d", "k_form_factor_2d_adj", "k_ff2d_lines_adj", "k_fe_prepare", "k_fe_vectors", "k_fused_prep",
            "k_fused_finish")
_FAMILY = re.compile(r"^(%s|k_wgemm\w*)(<|$)" % "|".join(FAMILIES))

CASES = [
    ({'n_ion': 1, 'fe': True, 'nvx': 320}, 2, 'lgfe', 0, ('k_fe_vectors<1>', 'k_wgemm<2>', 'k_spectrum<1, 1, 2, 256, true>', 'k_wgemm_t')),
    ({'n_ion': 1, 'fe': True, 'ppp': 5}, 2, 'lgfe', 0, ('k_fe_vectors<1>', 'k_wgemm<2>', 'k_spectrum<1, 1, 2, 512, true>', 'k_wgemm_t')),
    ({'n_ion': 1, 'fe': True}, 2, 'lgfe', 0, ('k_fe_vectors<1>', 'k_wgemm<2>', 'k_spectrum<1, 1, 2, 256, false>', 'k_wgemm_t')),
    ({'n_ion': 2, 'fe': True, 'nvx': 320}, 2, 'lgfe', 0, ('k_fe_vectors<2>', 'k_wgemm<2>', 'k_spectrum<2, 1, 2, 256, true>', 'k_wgemm_t')),
    ({'n_ion': 2, 'fe': True, 'ppp': 5}, 2, 'lgfe', 0, ('k_fe_vectors<2>', 'k_wgemm<2>', 'k_spectrum<2, 1, 2, 512, true>', 'k_wgemm_t')),
    ({'n_ion': 2, 'fe': True}, 2, 'lgfe', 0, ('k_fe_vectors<2>', 'k_wgemm<2>', 'k_spectrum<2, 1, 2, 256, false>', 'k_wgemm_t')),
    ({'n_ion': 3, 'fe': True, 'nvx': 320}, 2, 'lgfe', 0, ('k_fe_vectors<3>', 'k_wgemm<2>', 'k_spectrum<3, 1, 2, 256, true>', 'k_wgemm_t')),
    ({'n_ion': 3, 'fe': True, 'ppp': 5}, 2, 'lgfe', 0, ('k_fe_vectors<3>', 'k_wgemm<2>', 'k_spectrum<3, 1, 2, 512, true>', 'k_wgemm_t')),
    ({'n_ion': 3, 'fe': True}, 2, 'lgfe', 0, ('k_fe_vectors<3>', 'k_wgemm<2>', 'k_spectrum<3, 1, 2, 256, false>', 'k_wgemm_t')),
    ({'n_ion': 4, 'fe': True, 'nvx': 320}, 2, 'lgfe', 0, ('k_fe_vectors<4>', 'k_wgemm<2>', 'k_spectrum<4, 1, 2, 256, true>', 'k_wgemm_t')),
    ({'n_ion': 4, 'fe': True, 'ppp': 5}, 2, 'lgfe', 0, ('k_fe_vectors<4>', 'k_wgemm<2>', 'k_spectrum<4, 1, 2, 512, true>', 'k_wgemm_t')),
    ({'n_ion': 4, 'fe': True}, 2, 'lgfe', 0, ('k_fe_vectors<4>', 'k_wgemm<2>', 'k_spectrum<4, 1, 2, 256, false>', 'k_wgemm_t')),
    ({'n_ion': 1, 'm': True, 'nvx': 192}, 2, 'lg', 32, ('k_fe_vectors<1>', 'k_wgemm<4>', 'k_fused_prep<1>', 'k_spectrum_fused<1, 1, true, true>', 'k_fused_finish<1>')),
    ({'n_ion': 1, 'm': True, 'ppp': 2, 'nvx': 256}, 2, 'lg', 0, ('k_fe_vectors<1>', 'k_wgemm_w', 'k_spectrum_rows<1, 1, true, true, false>')),
    ({'n_ion': 1, 'm': True, 'nvx': 384}, 2, 'lg', 0, ('k_fe_vectors<1>', 'k_wgemm_w', 'k_fused_prep<1>', 'k_spectrum_fused<1, 1, true, false>', 'k_fused_finish<1>')),
    ({'n_ion': 1, 'm': True, 'ppp': 2, 'nvx': 448}, 2, 'lg', 0, ('k_fe_vectors<1>', 'k_wgemm_w', 'k_spectrum_rows<1, 1, true, false, false>')),
    ({'n_ion': 1, 'm': True, 'nvx': 512}, 2, 'lg', 0, ('k_fe_vectors<1>', 'k_wgemm_w', 'k_spectrum<1, 1, 1, 256, true>')),
    ({'n_ion': 1, 'm': True, 'ppp': 2}, 2, 'lg', 0, ('k_fe_vectors<1>', 'k_wgemm_w', 'k_spectrum_rows<1, 1, false, true, false>')),
    ({'n_ion': 1, 'm': True, 'ppp': 2}, 2, 'lg', 8, ('k_fe_vectors<1>', 'k_wgemm_w', 'k_spectrum_rows<1, 1, false, false, false>')),
    ({'n_ion': 1, 'm': True, 'ppp': 5, 'sde': 4.0}, 2, 'lg', 0, ('k_fe_vectors<1>', 'k_wgemm_w', 'k_spectrum<1, 1, 1, 512, true>')),
    ({'n_ion': 1, 'm': True}, 2, 'lg', 0, ('k_fe_vectors<1>', 'k_wgemm_w', 'k_fused_prep<1>', 'k_spectrum_fused<1, 1, false, true>', 'k_fused_finish<1>')),
    ({'n_ion': 1, 'm': True}, 2, 'lg', 1, ('k_fe_vectors<1>', 'k_wgemm_w', 'k_spectrum<1, 1, 1, 256, false>')),
    ({'n_ion': 1, 'm': True}, 2, 'lg', 8, ('k_fe_vectors<1>', 'k_wgemm_w', 'k_fused_prep<1>', 'k_spectrum_fused<1, 1, false, false>', 'k_fused_finish<1>')),
    ({'n_ion': 2, 'm': True, 'nvx': 192}, 2, 'lg', 0, ('k_fe_vectors<2>', 'k_wgemm_w', 'k_fused_prep<2>', 'k_spectrum_fused<2, 1, true, true>', 'k_fused_finish<2>')),
    ({'n_ion': 2, 'm': True, 'ppp': 2, 'nvx': 256}, 2, 'lg', 0, ('k_fe_vectors<2>', 'k_wgemm_w', 'k_spectrum_rows<2, 1, true, true, false>')),
    ({'n_ion': 2, 'm': True, 'nvx': 384}, 2, 'lg', 0, ('k_fe_vectors<2>', 'k_wgemm_w', 'k_fused_prep<2>', 'k_spectrum_fused<2, 1, true, false>', 'k_fused_finish<2>')),
    ({'n_ion': 2, 'm': True, 'ppp': 2, 'nvx': 448}, 2, 'lg', 0, ('k_fe_vectors<2>', 'k_wgemm_w', 'k_spectrum_rows<2, 1, true, false, false>')),
    ({'n_ion': 2, 'm': True, 'nvx': 512}, 2, 'lg', 0, ('k_fe_vectors<2>', 'k_wgemm_w', 'k_spectrum<2, 1, 1, 256, true>')),
    ({'n_ion': 2, 'm': True, 'ppp': 2}, 2, 'lg', 0, ('k_fe_vectors<2>', 'k_wgemm_w', 'k_spectrum_rows<2, 1, false, true, false>')),
    ({'n_ion': 2, 'm': True, 'ppp': 2}, 2, 'lg', 8, ('k_fe_vectors<2>', 'k_wgemm_w', 'k_spectrum_rows<2, 1, false, false, false>')),
    ({'n_ion': 2, 'm': True, 'ppp': 5, 'sde': 4.0}, 2, 'lg', 0, ('k_fe_vectors<2>', 'k_wgemm_w', 'k_spectrum<2, 1, 1, 512, true>')),
    ({'n_ion': 2, 'm': True}, 2, 'lg', 0, ('k_fe_vectors<2>', 'k_wgemm_w', 'k_fused_prep<2>', 'k_spectrum_fused<2, 1, false, true>', 'k_fused_finish<2>')),
    ({'n_ion': 2, 'm': True}, 2, 'lg', 1, ('k_fe_vectors<2>', 'k_wgemm_w', 'k_spectrum<2, 1, 1, 256, false>')),
    ({'n_ion': 2, 'm': True}, 2, 'lg', 8, ('k_fe_vectors<2>', 'k_wgemm_w', 'k_fused_prep<2>', 'k_spectrum_fused<2, 1, false, false>', 'k_fused_finish<2>')),
    ({'n_ion': 3, 'm': True, 'nvx': 1024}, 2, 'lg', 0, ('k_fe_vectors<3>', 'k_wgemm_w', 'k_spectrum<3, 1, 1, 256, true>')),
    ({'n_ion': 3, 'm': True, 'ppp': 5}, 2, 'lg', 0, ('k_fe_vectors<3>', 'k_wgemm_w', 'k_spectrum<3, 1, 1, 512, true>')),
    ({'n_ion': 3, 'm': True}, 2, 'lg', 0, ('k_fe_vectors<3>', 'k_wgemm_w', 'k_spectrum<3, 1, 1, 256, false>')),
    ({'n_ion': 4, 'm': True, 'nvx': 1024}, 2, 'lg', 0, ('k_fe_vectors<4>', 'k_wgemm_w', 'k_spectrum<4, 1, 1, 256, true>')),
    ({'n_ion': 4, 'm': True, 'ppp': 5}, 2, 'lg', 0, ('k_fe_vectors<4>', 'k_wgemm_w', 'k_spectrum<4, 1, 1, 512, true>')),
    ({'n_ion': 4, 'm': True}, 2, 'lg', 0, ('k_fe_vectors<4>', 'k_wgemm_w', 'k_spectrum<4, 1, 1, 256, false>')),
    ({'n_ion': 1, 'nvx': 640, 'nang': 17}, 2, 'fwd', 0, ('k_forward_pairs<1, true, 0, 1>',)),
    ({'n_ion': 1, 'nvx': 640, 'nang': 17}, 2, 'lg', 0, ('k_fused_prep<1>', 'k_spectrum_fused<1, 0, true, false>', 'k_fused_finish<1>')),
    ({'n_ion': 1, 'nang': 17}, 2, 'fwd', 0, ('k_forward_pairs<1, false, 0, 1>',)),
    ({'n_ion': 1, 'nang': 17}, 2, 'lg', 0, ('k_fused_prep<1>', 'k_spectrum_fused<1, 0, false, false>', 'k_fused_finish<1>')),
    ({'n_ion': 1, 'nang': 17}, 600, 'fwd', 0, ('k_fused_prep<1>', 'k_forward_pairs<1, true, 0, 2>')),
    ({'n_ion': 1, 'ppp': 5, 'nvx': 256}, 2, 'fwd', 0, ('k_spectrum_rows<1, 0, true, true, true>',)),
    ({'n_ion': 1, 'ppp': 5, 'nvx': 256}, 2, 'lg', 0, ('k_spectrum_rows<1, 0, true, true, false>',)),
    ({'n_ion': 1, 'nvx': 256}, 2, 'lg', 0, ('k_fused_prep<1>', 'k_spectrum_fused<1, 0, true, true>', 'k_fused_finish<1>')),
    ({'n_ion': 1, 'nvx': 320}, 2, 'fwd', 0, ('k_forward_pairs<1, true, 2, 1>',)),
    ({'n_ion': 1, 'nvx': 320}, 2, 'fwd', 1, ('k_fused_prep<1>', 'k_forward_pairs<1, true, 1, 2>')),
    ({'n_ion': 1, 'nvx': 320}, 2, 'lg', 1, ('k_spectrum<1, 1, 0, 256, true>',)),
    ({'n_ion': 1, 'ppp': 5, 'nvx': 640}, 2, 'fwd', 0, ('k_spectrum_rows<1, 0, true, false, true>',)),
    ({'n_ion': 1, 'ppp': 5, 'nvx': 640}, 2, 'lg', 0, ('k_spectrum_rows<1, 0, true, false, false>',)),
    ({'n_ion': 1, 'ppp': 2}, 2, 'fwd', 0, ('k_spectrum_rows<1, 0, false, true, true>',)),
    ({'n_ion': 1, 'ppp': 2}, 2, 'lg', 0, ('k_spectrum_rows<1, 0, false, true, false>',)),
    ({'n_ion': 1, 'ppp': 2}, 2, 'al', 0, ('k_spectrum<1, 2, 0, 256, true>',)),
    ({'n_ion': 1, 'ppp': 2}, 2, 'fwd', 2, ('k_spectrum<1, 0, 0, 256, true>',)),
    ({'n_ion': 1, 'ppp': 2}, 2, 'fwd', 8, ('k_spectrum_rows<1, 0, false, false, true>',)),
    ({'n_ion': 1, 'ppp': 2}, 2, 'lg', 8, ('k_spectrum_rows<1, 0, false, false, false>',)),
    ({'n_ion': 1, 'ppp': 5, 'sde': 4.0}, 2, 'fwd', 0, ('k_spectrum<1, 0, 0, 512, true>',)),
    ({'n_ion': 1, 'ppp': 5, 'sde': 4.0}, 2, 'lg', 0, ('k_spectrum<1, 1, 0, 512, true>',)),
    ({'n_ion': 1, 'ppp': 5}, 2, 'al', 0, ('k_spectrum<1, 2, 0, 512, true>',)),
    ({'n_ion': 1}, 2, 'fwd', 0, ('k_forward_pairs<1, false, 2, 1>',)),
    ({'n_ion': 1}, 2, 'lg', 0, ('k_fused_prep<1>', 'k_spectrum_fused<1, 0, false, true>', 'k_fused_finish<1>')),
    ({'n_ion': 1}, 2, 'al', 0, ('k_spectrum<1, 2, 0, 256, false>',)),
    ({'n_ion': 1}, 2, 'fwd', 1, ('k_fused_prep<1>', 'k_forward_pairs<1, false, 1, 2>')),
    ({'n_ion': 1}, 2, 'lg', 1, ('k_spectrum<1, 1, 0, 256, false>',)),
    ({'n_ion': 1}, 2, 'fwd', 9, ('k_fused_prep<1>', 'k_forward_pairs<1, false, 0, 2>')),
    ({'n_ion': 1}, 2, 'fwd', 256, ('k_spectrum<1, 0, 0, 256, false>',)),
    ({'n_ion': 1}, 600, 'fwd', 0, ('k_fused_prep<1>', 'k_forward_pairs<1, true, 2, 2>')),
    ({'n_ion': 2, 'nvx': 640, 'nang': 17}, 2, 'fwd', 0, ('k_forward_pairs<2, true, 0, 1>',)),
    ({'n_ion': 2, 'nvx': 640, 'nang': 17}, 2, 'lg', 0, ('k_fused_prep<2>', 'k_spectrum_fused<2, 0, true, false>', 'k_fused_finish<2>')),
    ({'n_ion': 2, 'nang': 17}, 2, 'fwd', 0, ('k_forward_pairs<2, false, 0, 1>',)),
    ({'n_ion': 2, 'nang': 17}, 2, 'lg', 0, ('k_fused_prep<2>', 'k_spectrum_fused<2, 0, false, false>', 'k_fused_finish<2>')),
    ({'n_ion': 2, 'nang': 17}, 600, 'fwd', 0, ('k_fused_prep<2>', 'k_forward_pairs<2, true, 0, 2>')),
    ({'n_ion': 2, 'ppp': 5, 'nvx': 256}, 2, 'fwd', 0, ('k_spectrum_rows<2, 0, true, true, true>',)),
    ({'n_ion': 2, 'ppp': 5, 'nvx': 256}, 2, 'lg', 0, ('k_spectrum_rows<2, 0, true, true, false>',)),
    ({'n_ion': 2, 'nvx': 256}, 2, 'lg', 0, ('k_fused_prep<2>', 'k_spectrum_fused<2, 0, true, true>', 'k_fused_finish<2>')),
    ({'n_ion': 2, 'nvx': 320}, 2, 'fwd', 0, ('k_forward_pairs<2, true, 2, 1>',)),
    ({'n_ion': 2, 'nvx': 320}, 2, 'fwd', 1, ('k_fused_prep<2>', 'k_forward_pairs<2, true, 1, 2>')),
    ({'n_ion': 2, 'nvx': 320}, 2, 'lg', 1, ('k_spectrum<2, 1, 0, 256, true>',)),
    ({'n_ion': 2, 'ppp': 5, 'nvx': 640}, 2, 'fwd', 0, ('k_spectrum_rows<2, 0, true, false, true>',)),
    ({'n_ion': 2, 'ppp': 5, 'nvx': 640}, 2, 'lg', 0, ('k_spectrum_rows<2, 0, true, false, false>',)),
    ({'n_ion': 2, 'ppp': 2}, 2, 'fwd', 0, ('k_spectrum_rows<2, 0, false, true, true>',)),
    ({'n_ion': 2, 'ppp': 2}, 2, 'lg', 0, ('k_spectrum_rows<2, 0, false, true, false>',)),
    ({'n_ion': 2, 'ppp': 2}, 2, 'al', 0, ('k_spectrum<2, 2, 0, 256, true>',)),
    ({'n_ion': 2, 'ppp': 2}, 2, 'fwd', 2, ('k_spectrum<2, 0, 0, 256, true>',)),
    ({'n_ion': 2, 'ppp': 2}, 2, 'fwd', 8, ('k_spectrum_rows<2, 0, false, false, true>',)),
    ({'n_ion': 2, 'ppp': 2}, 2, 'lg', 8, ('k_spectrum_rows<2, 0, false, false, false>',)),
    ({'n_ion': 2, 'ppp': 5, 'sde': 4.0}, 2, 'fwd', 0, ('k_spectrum<2, 0, 0, 512, true>',)),
    ({'n_ion': 2, 'ppp': 5, 'sde': 4.0}, 2, 'lg', 0, ('k_spectrum<2, 1, 0, 512, true>',)),
    ({'n_ion': 2, 'ppp': 5}, 2, 'al', 0, ('k_spectrum<2, 2, 0, 512, true>',)),
    ({'n_ion': 2}, 2, 'fwd', 0, ('k_forward_pairs<2, false, 2, 1>',)),
    ({'n_ion': 2}, 2, 'lg', 0, ('k_fused_prep<2>', 'k_spectrum_fused<2, 0, false, true>', 'k_fused_finish<2>')),
    ({'n_ion': 2}, 2, 'al', 0, ('k_spectrum<2, 2, 0, 256, false>',)),
    ({'n_ion': 2}, 2, 'fwd', 1, ('k_fused_prep<2>', 'k_forward_pairs<2, false, 1, 2>')),
    ({'n_ion': 2}, 2, 'lg', 1, ('k_spectrum<2, 1, 0, 256, false>',)),
    ({'n_ion': 2}, 2, 'fwd', 9, ('k_fused_prep<2>', 'k_forward_pairs<2, false, 0, 2>')),
    ({'n_ion': 2}, 2, 'fwd', 256, ('k_spectrum<2, 0, 0, 256, false>',)),
    ({'n_ion': 2}, 600, 'fwd', 0, ('k_fused_prep<2>', 'k_forward_pairs<2, true, 2, 2>')),
    ({'n_ion': 3, 'ppp': 2}, 2, 'fwd', 0, ('k_spectrum<3, 0, 0, 256, true>',)),
    ({'n_ion': 3, 'ppp': 2}, 2, 'lg', 0, ('k_spectrum<3, 1, 0, 256, true>',)),
    ({'n_ion': 3, 'ppp': 2}, 2, 'al', 0, ('k_spectrum<3, 2, 0, 256, true>',)),
    ({'n_ion': 3, 'ppp': 5}, 2, 'fwd', 0, ('k_spectrum<3, 0, 0, 512, true>',)),
    ({'n_ion': 3, 'ppp': 5}, 2, 'lg', 0, ('k_spectrum<3, 1, 0, 512, true>',)),
    ({'n_ion': 3, 'ppp': 5}, 2, 'al', 0, ('k_spectrum<3, 2, 0, 512, true>',)),
    ({'n_ion': 3}, 2, 'fwd', 0, ('k_spectrum<3, 0, 0, 256, false>',)),
    ({'n_ion': 3}, 2, 'lg', 0, ('k_spectrum<3, 1, 0, 256, false>',)),
    ({'n_ion': 3}, 2, 'al', 0, ('k_spectrum<3, 2, 0, 256, false>',)),
    ({'n_ion': 4, 'ppp': 2}, 2, 'fwd', 0, ('k_spectrum<4, 0, 0, 256, true>',)),
    ({'n_ion': 4, 'ppp': 2}, 2, 'lg', 0, ('k_spectrum<4, 1, 0, 256, true>',)),
    ({'n_ion': 4, 'ppp': 2}, 2, 'al', 0, ('k_spectrum<4, 2, 0, 256, true>',)),
    ({'n_ion': 4, 'ppp': 5}, 2, 'fwd', 0, ('k_spectrum<4, 0, 0, 512, true>',)),
    ({'n_ion': 4, 'ppp': 5}, 2, 'lg', 0, ('k_spectrum<4, 1, 0, 512, true>',)),
    ({'n_ion': 4, 'ppp': 5}, 2, 'al', 0, ('k_spectrum<4, 2, 0, 512, true>',)),
    ({'n_ion': 4}, 2, 'fwd', 0, ('k_spectrum<4, 0, 0, 256, false>',)),
    ({'n_ion': 4}, 2, 'lg', 0, ('k_spectrum<4, 1, 0, 256, false>',)),
    ({'n_ion': 4}, 2, 'al', 0, ('k_spectrum<4, 2, 0, 256, false>',)),
    ({'n_ion': 1}, 2, 'chi', 0, ('k_fe_prepare<1>',)),
    ({'n_ion': 1}, 2, 'ff', 0, ('k_form_factor<1>',)),
    ({'n_ion': 1}, 2, 'ffg', 0, ('k_form_factor_adj<1, 0>', 'k_ff2d_lines_adj<1>')),
    ({'n_ion': 1, 'fe': True}, 2, 'ffg_fe', 0, ('k_fe_vectors<1>', 'k_wgemm<2>', 'k_form_factor_adj<1, 2>', 'k_ff2d_lines_adj<1>', 'k_wgemm_t')),
    ({'n_ion': 1}, 2, 'ff2d_fwd_lds', 0, ('k_form_factor_2d<1, true, 4, false>',)),
    ({'n_ion': 1}, 2, 'ff2d_save_lds', 0, ('k_form_factor_2d<1, true, 4, true>',)),
    ({'n_ion': 1}, 2, 'ff2d_adj_lds', 0, ('k_form_factor_2d_adj<1, true, 4>', 'k_ff2d_lines_adj<1>')),
    ({'n_ion': 1}, 2, 'ff2d_fwd_l2', 0, ('k_form_factor_2d<1, false, 1, false>',)),
    ({'n_ion': 1}, 2, 'ff2d_save_l2', 0, ('k_form_factor_2d<1, false, 1, true>',)),
    ({'n_ion': 1}, 2, 'ff2d_adj_l2', 0, ('k_form_factor_2d_adj<1, false, 1>', 'k_ff2d_lines_adj<1>')),
    ({'n_ion': 2}, 2, 'chi', 0, ('k_fe_prepare<2>',)),
    ({'n_ion': 2}, 2, 'ff', 0, ('k_form_factor<2>',)),
    ({'n_ion': 2}, 2, 'ffg', 0, ('k_form_factor_adj<2, 0>', 'k_ff2d_lines_adj<2>')),
    ({'n_ion': 2, 'fe': True}, 2, 'ffg_fe', 0, ('k_fe_vectors<2>', 'k_wgemm<2>', 'k_form_factor_adj<2, 2>', 'k_ff2d_lines_adj<2>', 'k_wgemm_t')),
    ({'n_ion': 2}, 2, 'ff2d_fwd_lds', 0, ('k_form_factor_2d<2, true, 4, false>',)),
    ({'n_ion': 2}, 2, 'ff2d_save_lds', 0, ('k_form_factor_2d<2, true, 4, true>',)),
    ({'n_ion': 2}, 2, 'ff2d_adj_lds', 0, ('k_form_factor_2d_adj<2, true, 4>', 'k_ff2d_lines_adj<2>')),
    ({'n_ion': 2}, 2, 'ff2d_fwd_l2', 0, ('k_form_factor_2d<2, false, 1, false>',)),
    ({'n_ion': 2}, 2, 'ff2d_save_l2', 0, ('k_form_factor_2d<2, false, 1, true>',)),
    ({'n_ion': 2}, 2, 'ff2d_adj_l2', 0, ('k_form_factor_2d_adj<2, false, 1>', 'k_ff2d_lines_adj<2>')),
    ({'n_ion': 3}, 2, 'chi', 0, ('k_fe_prepare<3>',)),
    ({'n_ion': 3}, 2, 'ff', 0, ('k_form_factor<3>',)),
    ({'n_ion': 3}, 2, 'ffg', 0, ('k_form_factor_adj<3, 0>', 'k_ff2d_lines_adj<3>')),
    ({'n_ion': 3, 'fe': True}, 2, 'ffg_fe', 0, ('k_fe_vectors<3>', 'k_wgemm<2>', 'k_form_factor_adj<3, 2>', 'k_ff2d_lines_adj<3>', 'k_wgemm_t')),
    ({'n_ion': 3}, 2, 'ff2d_fwd_lds', 0, ('k_form_factor_2d<3, true, 4, false>',)),
    ({'n_ion': 3}, 2, 'ff2d_save_lds', 0, ('k_form_factor_2d<3, true, 4, true>',)),
    ({'n_ion': 3}, 2, 'ff2d_adj_lds', 0, ('k_form_factor_2d_adj<3, true, 4>', 'k_ff2d_lines_adj<3>')),
    ({'n_ion': 3}, 2, 'ff2d_fwd_l2', 0, ('k_form_factor_2d<3, false, 1, false>',)),
    ({'n_ion': 3}, 2, 'ff2d_save_l2', 0, ('k_form_factor_2d<3, false, 1, true>',)),
    ({'n_ion': 3}, 2, 'ff2d_adj_l2', 0, ('k_form_factor_2d_adj<3, false, 1>', 'k_ff2d_lines_adj<3>')),
    ({'n_ion': 4}, 2, 'chi', 0, ('k_fe_prepare<4>',)),
    ({'n_ion': 4}, 2, 'ff', 0, ('k_form_factor<4>',)),
    ({'n_ion': 4}, 2, 'ffg', 0, ('k_form_factor_adj<4, 0>', 'k_ff2d_lines_adj<4>')),
    ({'n_ion': 4, 'fe': True}, 2, 'ffg_fe', 0, ('k_fe_vectors<4>', 'k_wgemm<2>', 'k_form_factor_adj<4, 2>', 'k_ff2d_lines_adj<4>', 'k_wgemm_t')),
    ({'n_ion': 4}, 2, 'ff2d_fwd_lds', 0, ('k_form_factor_2d<4, true, 4, false>',)),
    ({'n_ion': 4}, 2, 'ff2d_save_lds', 0, ('k_form_factor_2d<4, true, 4, true>',)),
    ({'n_ion': 4}, 2, 'ff2d_adj_lds', 0, ('k_form_factor_2d_adj<4, true, 4>', 'k_ff2d_lines_adj<4>')),
    ({'n_ion': 4}, 2, 'ff2d_fwd_l2', 0, ('k_form_factor_2d<4, false, 1, false>',)),
    ({'n_ion': 4}, 2, 'ff2d_save_l2', 0, ('k_form_factor_2d<4, false, 1, true>',)),
    ({'n_ion': 4}, 2, 'ff2d_adj_l2', 0, ('k_form_factor_2d_adj<4, false, 1>', 'k_ff2d_lines_adj<4>')),
    # trainable Z of every species and a tied Ti (ion-3 to ion-1) on 3- and 4-species decks: every gradient column per lineout
    ({'n_ion': 3, 'z': True}, 2, 'lg', 0, ('k_spectrum<3, 1, 0, 256, false>',)),
    ({'n_ion': 4, 'z': True}, 2, 'lg', 0, ('k_spectrum<4, 1, 0, 256, false>',)),
    ({'n_ion': 3, 'z': True, 'tie': True}, 2, 'lg', 0, ('k_spectrum<3, 1, 0, 256, false>',)),
    ({'n_ion': 3, 'z': True, 'tie': True}, 2, 'fwd', 0, ('k_spectrum<3, 0, 0, 256, false>',)),
    ({'n_ion': 4, 'z': True, 'tie': True}, 2, 'lg', 2, ('k_spectrum<4, 1, 0, 256, false>',)),
    ({'n_ion': 3, 'z': True, 'fe': True}, 2, 'lgfe', 0, ('k_fe_vectors<3>', 'k_spectrum<3, 1, 2, 256, false>', 'k_wgemm_t')),
    ({'n_ion': 4, 'z': True, 'fe': True, 'tie': True}, 2, 'lgfe', 0, ('k_fe_vectors<4>', 'k_spectrum<4, 1, 2, 256, false>', 'k_wgemm_t')),
    ({'n_ion': 3, 'z': True, 'm': True, 'tie': True}, 2, 'lg', 0, ('k_fe_vectors<3>', 'k_spectrum<3, 1, 1, 256, false>')),
    ({'n_ion': 4, 'z': True, 'm': True}, 2, 'lg', 0, ('k_fe_vectors<4>', 'k_spectrum<4, 1, 1, 256, false>')),
]

def _case_id(c):
    d, B, entry, plan, _ = c
    return "-".join([entry] + [f"{k}{v}" for k, v in sorted(d.items())] + [f"B{B}", f"plan{plan}"])


def _library_kernels(lib_path):
    """Kernel names in the library's embedded code object, demangled, without 'void tsff::'."""
    data = open(lib_path, "rb").read()
    mangled = {m.decode() for m in re.findall(rb"_ZN4tsff\d+k_\w+", data)}
    mangled = sorted({m[:-3] if m.endswith(".kd") else m for m in mangled})
    out = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.split("\n")
    return {re.sub(r"^(void )?tsff::", "", s).split("(")[0] for s in out if s.strip()}


@pytest.fixture(scope="module")
def lib():
    from tsadar_amd import build, _lib

    build.build()
    return _lib.load()


def test_every_instantiation_has_a_case(lib):
    from tsadar_amd import build

    shipped = _library_kernels(build.OUT)
    contract = {k for k in shipped if _FAMILY.match(k)}
    named = {k for c in CASES for k in c[4]}
    assert len(contract) == 174, f"{len(contract)} instantiations in the contract families (174 when the contract was written)"
    missing = sorted(contract - named)
    assert not missing, f"{len(missing)} shipped instantiations have no case in CASES: {missing}"
    unknown = sorted(named - shipped)
    assert not unknown, f"CASES names kernels the library does not contain: {unknown}"
    assert len({_case_id(c) for c in CASES}) == len(CASES)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: every case against its reference
# ---------------------------------------------------------------------------------------------------------------------

def _deck(d):
    n = d.get("n_ion", 1)
    active = ("Te", "ne", "Ti", "lam", "amp1") + (("m",) if d.get("m") else ()) + (("Z",) if d.get("z") else ()) + \
        (("Ti_same_3",) if d.get("tie") else ())
    cfg = decks.deck_fit(points_per_pixel=d.get("ppp", 1), nvx=d.get("nvx", 128), active=active, n_ion=n)
    if d.get("G", 1) > 1:
        g = cfg["parameters"]["general"]
        g["Te_gradient"].update(val=3.0, num_grad_points=d["G"])
        g["ne_gradient"].update(val=4.0, num_grad_points=d["G"])
    w = cfg["other"]["PhysParams"]["widIRF"]
    if "sde" in d:
        w["spect_stddev_ele"] = d["sde"]
    if "sdi" in d:
        w["spect_stddev_ion"] = d["sdi"]
    return cfg


_ENGINES = {}


def _engine(d, cfg, B):
    """One engine per deck: the cases of a deck differ only in B, entry point and plan (CASES is grouped by deck)."""
    from tsadar_amd import _lib as L
    from tsadar_amd.engine import Engine

    key = repr(sorted(d.items()))
    if key not in _ENGINES:
        _ENGINES.clear()
        Bmax = max(c[1] for c in CASES if c[0] == d)
        nang = d.get("nang", 10)
        sa = dict(sa=np.linspace(53.6, 66.1, nang), weights=np.ones((Bmax, nang)) / nang)
        _ENGINES[key] = (Engine(cfg, sa, fe_mode=L.FE_PER_LINEOUT if d.get("fe") else None), sa)
    eng, sa = _ENGINES[key]
    return eng, dict(sa=sa["sa"], weights=sa["weights"][:B])


def _sync():
    import torch

    torch.cuda.synchronize()


def _assert_launched(eng, kernels):
    got = eng.last_launch()
    missing = [k for k in kernels if k not in got]
    assert not missing, f"expected {missing} among the launched kernels {got}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_case_matches_reference(case):
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    d, B, entry, plan, kernels = case
    cfg = _deck(d)
    eng, sa = _engine(d, cfg, B)
    eng.set_launch_plan(plan)
    n_ion = d.get("n_ion", 1)
    if entry == "chi":
        _chi_case(eng, kernels)
    elif entry.startswith("ff2d"):
        _ff2d_case(eng, cfg, sa, B, entry, kernels, n_ion)
    elif entry.startswith("ff"):
        _ff_case(eng, cfg, sa, B, entry, kernels, n_ion)
    else:
        _spectrum_case(eng, cfg, sa, d, B, entry, kernels, n_ion)


def _free_form_fe(B, nvx, seed):
    rng = np.random.default_rng(seed)
    vx = orc.velocity_grid(nvx)
    fes = []
    for b in range(B):
        f = orc.dlm_fe(rng.uniform(2.0, 3.5), nvx) * np.exp(0.15 * np.sin(1.3 * vx + rng.uniform(0, 6.28)) + 0.05 * np.tanh(vx))
        fes.append(f / np.sum(f) / (vx[1] - vx[0]))
    return np.stack(fes)


def _cheap_batch(B):
    """data of a large batch without B oracle evaluations: smooth positive spectra"""
    rng = np.random.default_rng(B)
    x = np.linspace(0, 1, 1024)
    E = 0.2 + np.exp(-(((x[None] - rng.uniform(0.2, 0.8, (B, 1))) / 0.1) ** 2))
    I = 0.1 + np.exp(-(((x[None] - 0.5) / 0.05) ** 2)) * rng.uniform(0.5, 1.5, (B, 1))
    return dict(e_data=E, i_data=I, e_amps=E.max(axis=1), i_amps=I.max(axis=1), noise_e=0.01 * np.ones((B, 1024)),
                noise_i=0.01 * np.ones((B, 1024)))


def _sub(tree_, rows):
    return {k: (v[rows] if isinstance(v, np.ndarray) and v.ndim >= 1 else v) for k, v in tree_.items()}


def _sensitivity_guard(cfg, sa, normed, batch, tol):
    """A kernel that drops or swaps a species must fail: changing any species' fraction by 1e-3 moves the oracle's ThryI
    by more than 100x the tolerance the case applies to ThryI."""
    n_ion = sum(1 for k in cfg["parameters"] if k.startswith("ion-"))
    _, I0, _, _ = orc.ts_diag(cfg, sa, normed, batch)
    for s in range(1, n_ion + 1):
        n2 = dict(normed)
        n2[f"fract_{s}"] = normed[f"fract_{s}"] + 1e-3
        _, I1, _, _ = orc.ts_diag(cfg, sa, n2, batch)
        assert util.rel_err(I1, I0) > 100 * tol, (s, util.rel_err(I1, I0))


def _trained(eng, n_ion):
    """names of the trainable leaves (a tied Ti is not one)"""
    names = ["Te", "ne", "m", "lam", "amp1"] + [f"{k}_{s}" for s in range(1, n_ion + 1) for k in ("Ti", "Z")]
    return [k for k in names if eng.slots.active[util.slot_of(k)]]


def _spectrum_inputs(eng, cfg, sa, d, B, n_ion, round_=0):
    """the batch, normalised leaves (round_ > 0: another seeded draw), parameter matrix and free-form f_e of a spectrum case"""
    batch = util.synthetic_batch(cfg, sa, B, seed=3 + B) if B <= 8 else _cheap_batch(B)
    normed = util.random_lineouts(cfg, B, seed=11 + n_ion + 100 * round_, ranges=dict(m=(2.1, 4.2)) if d.get("m") else None)
    X = util.normed_to_matrix(normed, n_ion)
    fe = _free_form_fe(B, eng.nvx, 5 + round_) if d.get("fe") else None
    return batch, normed, X, fe


def _spectrum_case(eng, cfg, sa, d, B, entry, kernels, n_ion):
    batch, normed, X, fe = _spectrum_inputs(eng, cfg, sa, d, B, n_ion)
    i_norm, e_norm = orc.loss_norms(cfg, batch)
    w = eng.loss_weights(B, i_norm, e_norm, cfg["data"]["ion_loss_scale"])
    gm = eng.slots.active.astype(np.uint8)
    if entry in ("fwd", "al"):
        if entry == "fwd":
            E, I = eng.forward(X, batch["e_amps"], batch["i_amps"], batch["noise_e"], batch["noise_i"], fe=fe)
        else:
            _, _, _, E, I = eng.array_loss(X, batch, fe=fe)
        out = dict(E=E, I=I)
    elif entry == "lgfe":
        terms, grad, E, I, gfe = eng.loss_grad(X, batch, w, gm, fe=fe, want_spectra=True, want_fe_grad=True)
        out = dict(terms=terms, grad=grad, E=E, I=I, gfe=gfe)
    else:
        terms, grad, E, I = eng.loss_grad(X, batch, w, gm, want_spectra=True)
        out = dict(terms=terms, grad=grad, E=E, I=I)
    _sync()
    _assert_launched(eng, kernels)
    _spectrum_check(cfg, sa, d, B, entry, n_ion, eng, batch, normed, X, fe, w, gm, {k: v.cpu().numpy() for k, v in out.items()})


def _spectrum_check(cfg, sa, d, B, entry, n_ion, eng, batch, normed, X, fe, w, gm, out):
    """the outputs of a spectrum case (host arrays E, I and, for the loss entries, terms, grad, gfe) against the oracles"""
    from oracle import c_oracle as co
    from oracle import tsadar_oracle_torch as ot

    rows = np.arange(B) if B <= 8 else np.array([0, B // 2, B - 1])   # lineouts compared with the oracle
    nb, sb = _sub(normed, rows), _sub(batch, rows)
    sar = dict(sa=sa["sa"], weights=sa["weights"][rows])
    tolE, tolI = 1e-8, 1e-7
    E, I = out["E"], out["I"]
    if n_ion >= 3:
        _sensitivity_guard(cfg, sar, nb, sb, tolI)
    if entry in ("fwd", "al"):
        Eo, Io, _, _ = orc.ts_diag(cfg, sar, nb, sb, fe_batch=None if fe is None else fe[rows])
        assert util.rel_err(E[rows], Eo) < tolE
        assert util.rel_err(I[rows], Io) < tolI
        return
    i_norm, e_norm = orc.loss_norms(cfg, batch)
    terms, g = out["terms"], out["grad"]
    if entry == "lgfe":
        names = _trained(eng, n_ion)
        assert np.all(g[:, gm == 0] == 0.0)
        val, ref, ref_fe, Eo, Io = ot.value_and_grad_fe(cfg, sa, normed, batch, i_norm, e_norm, names, fe)
        assert util.rel_err(E, Eo) < tolE and util.rel_err(I, Io) < tolI
        assert abs(float(np.dot(terms, w)) - val) < 1e-9 * abs(val)
        G = util.matrix_to_named(g, names)
        scale = max(np.max(np.abs(v)) for v in ref.values())
        for k in names:
            assert np.max(np.abs(G[k] - ref[k])) / scale < 1e-7, k
        a, r = out["gfe"] * fe, ref_fe * fe   # as d loss / d ln fe: the tails of fe span 20 decades
        assert np.max(np.abs(a - r)) / np.max(np.abs(r)) < 1e-7
        return
    assert np.all(g[:, gm == 0] == 0.0)
    if d.get("m"):   # the DLM order is differentiated: the autodiff twin
        names = _trained(eng, n_ion)
        val, ref, Eo, Io = ot.value_and_grad(cfg, sa, normed, batch, i_norm, e_norm, names)
        assert util.rel_err(E, Eo) < tolE and util.rel_err(I, Io) < tolI
        assert abs(float(np.dot(terms, w)) - val) < 1e-9 * abs(val)
        G = util.matrix_to_named(g, names)
        scale = max(np.max(np.abs(v)) for v in ref.values())
        for k in names:
            assert np.max(np.abs(G[k] - ref[k])) / scale < 1e-7, k
        return
    # plasma parameters: the C++ dual-number oracle, every compared lineout, per column
    sums, gref, Eo, Io = co.loss_grad(cfg, sar, X[rows], sb, w=w, gmask=gm)
    assert util.rel_err(E[rows], Eo) < tolE and util.rel_err(I[rows], Io) < tolI
    if len(rows) == B:
        np.testing.assert_allclose(terms, sums.sum(axis=0), rtol=1e-9)
    for s in np.nonzero(gm)[0]:
        assert np.max(np.abs(g[rows, s] - gref[:, s])) <= 1e-6 * np.max(np.abs(gref[:, s])), s


def _chi_case(eng, kernels):
    fes = np.stack([orc.dlm_fe(m, eng.nvx) for m in (2.0, 3.7)])
    W = eng.chi_table(fes).cpu().numpy()
    _sync()
    _assert_launched(eng, kernels)
    vx = orc.velocity_grid(eng.nvx)
    for k in range(fes.shape[0]):
        Wo, _ = orc.chi_table(vx, fes[k])
        assert np.max(np.abs(W[k] - Wo)) / np.max(np.abs(Wo)) < 1e-11, k


def _phys(cfg, sa, B, n_ion, seed):
    normed = util.random_lineouts(cfg, B, seed=seed)
    phys = orc.physical_params(cfg["parameters"], normed, True)
    if n_ion >= 3:
        unit = dict(e_amps=np.ones(B), i_amps=np.ones(B), noise_e=np.zeros((B, 1024)), noise_i=np.zeros((B, 1024)))
        _sensitivity_guard(cfg, sa, normed, unit, 1e-7)
    return phys, util.normed_to_matrix(phys, n_ion)


def _best_fd(J, an, perturb, steps, jabs=0.0):
    """min over step sizes of (|an - central difference| - rounding floor) / |difference|: a sample that crosses a table
    node inside the step spoils the quotient (kinks of the table lookups); J is a sum of jabs worth of float64 terms --
    as in test_form_factor_grad_finite_differences"""
    tried = []
    for h in steps:
        fd = (J(*perturb(h)) - J(*perturb(-h))) / (2 * h)
        tried.append((np.max(np.abs(an - fd)) - 2e-15 * jabs / abs(h)) / max(np.max(np.abs(fd)), 1e-300))
    return min(tried)


def _fd_names(n_ion):
    # every species' Ti, Z and fraction (with one species the fraction cancels from the form factor: no derivative to check)
    return ["Te", "ne"] + [f"{k}_{s}" for s in range(1, n_ion + 1) for k in ("Ti", "Z") + (("fract",) if n_ion > 1 else ())]


def _ff_case(eng, cfg, sa, B, entry, kernels, n_ion):
    import torch

    phys, X = _phys(cfg, sa, B, n_ion, 31 + n_ion)
    nvx = eng.nvx
    vx = orc.velocity_grid(nvx)
    if entry == "ff":
        for feature, rng in ((0, cfg["other"]["lamrangE"]), (1, cfg["other"]["lamrangI"])):
            P = eng.form_factor(feature, X).cpu().numpy()
            _sync()
            _assert_launched(eng, kernels)
            for b in range(B):
                p = orc.lineout_params(phys, b, n_ion)
                Po, _ = orc.form_factor(rng, cfg["other"]["npts"], 0.0, sa["sa"], 1, p, vx, orc.dlm_fe(2.0, nvx))
                assert np.max(np.abs(P[b] - Po) / np.abs(Po)) < 1e-7, (feature, b)
        return
    # the adjoint: the VJP of the torch twin's form factor (reverse-mode autodiff, oracle/tsadar_oracle_torch.py) with a random seed
    from oracle import tsadar_oracle_torch as ot

    fe = _free_form_fe(B, nvx, 9) if entry == "ffg_fe" else None
    feature = 1
    rng = np.random.default_rng(7)
    P0 = eng.form_factor(feature, X, fe=fe)
    Pbar = torch.tensor(rng.standard_normal(tuple(P0.shape)), dtype=torch.float64, device=P0.device)
    gp, gf = eng.form_factor_grad(feature, X, fe, Pbar, want_fe=fe is not None)
    _sync()
    _assert_launched(eng, kernels)
    gp = gp.cpu().numpy()
    gf = gf.cpu().numpy() if gf is not None else None
    Pb = Pbar.cpu()
    scalars = ["Te", "ne", "lam", "ud", "Va"]
    G, R, RF = [], [], []
    for b in range(B):
        p = orc.lineout_params(phys, b, n_ion)
        pt = {k: torch.tensor(v, dtype=torch.float64, requires_grad=k in scalars) if not isinstance(v, list) else v for k, v in p.items()}
        for k in ("Ti", "Z", "fract"):
            pt[k] = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in p[k]]
        fb = torch.tensor(fe[b] if fe is not None else orc.dlm_fe(2.0, nvx), dtype=torch.float64, requires_grad=True)
        Pt, _ = ot.form_factor(cfg["other"]["lamrangI"], cfg["other"]["npts"], 0.0, sa["sa"], 1, pt, vx, fb, ot.chi_table(vx, fb))
        (Pt * Pb[b]).sum().backward()
        for k in scalars:
            G.append(gp[b, util.slot_of(k)]); R.append(float(pt[k].grad))
        for k in ("Ti", "Z", "fract"):
            for s_ in range(n_ion):
                G.append(gp[b, util.slot_of(f"{k}_{s_ + 1}")]); R.append(float(pt[k][s_].grad))
        if gf is not None:   # as d J / d ln fe: the tails of fe span 20 decades
            RF.append((gf[b] * fe[b], fb.grad.numpy() * fe[b]))
    G, R = np.array(G), np.array(R)
    assert np.max(np.abs(G - R)) <= 1e-7 * np.max(np.abs(R)), np.max(np.abs(G - R)) / np.max(np.abs(R))
    for a_, r_ in RF:
        assert np.max(np.abs(a_ - r_)) <= 1e-7 * np.max(np.abs(r_)), np.max(np.abs(a_ - r_)) / np.max(np.abs(r_))


def _fe2d(nv, width=1.3):
    vx = orc.velocity_grid(nv)
    X, Y = np.meshgrid(vx, vx, indexing="ij")
    f = np.exp(-((X / width) ** 2 + (Y / 0.8) ** 2) ** 1.4 / 2) + 0.05 * np.exp(-((X - 2.0) ** 2 + (Y + 1.0) ** 2))
    return vx, f / (f.sum() * (vx[1] - vx[0]) ** 2)


def _ff2d_case(eng, cfg, sa, B, entry, kernels, n_ion):
    import torch

    nv = 48 if entry.endswith("_lds") else 132
    phys, X = _phys(cfg, sa, B, n_ion, 61 + n_ion)
    vx, fe2 = _fe2d(nv)
    ud_ang, va_ang = 25.0, -40.0
    if not entry.startswith("ff2d_adj"):
        for feature in (0, 1):
            P = eng.form_factor_2d(feature, X, fe2, ud_ang, va_ang, save=entry.startswith("ff2d_save")).cpu().numpy()
            _sync()
            _assert_launched(eng, kernels)
            _ff2d_check_forward(cfg, sa, B, n_ion, phys, feature, nv, ud_ang, va_ang, P)
        return
    # the adjoint: directional derivatives of <Pbar, P> by central differences of the HIP 2-D forward
    feature = 1
    rng = np.random.default_rng(5)
    P0 = eng.form_factor_2d(feature, X, fe2, ud_ang, va_ang)
    Pbar = torch.tensor(rng.standard_normal(tuple(P0.shape)), dtype=torch.float64, device=P0.device)
    gp, gf = eng.form_factor_2d_grad(feature, X, fe2, Pbar, ud_ang, va_ang, want_table=True)
    _sync()
    _assert_launched(eng, kernels)
    _ff2d_check_adjoint(eng, X, fe2, Pbar, feature, ud_ang, va_ang, n_ion, gp.cpu().numpy(), gf.cpu().numpy())


def _ff2d_check_forward(cfg, sa, B, n_ion, phys, feature, nv, ud_ang, va_ang, P):
    """P [B, G, npts, n_angles] of tsff_form_factor_2d (host) against the oracle at four wavelengths"""
    rng = (cfg["other"]["lamrangE"], cfg["other"]["lamrangI"])[feature]
    vx, fe2 = _fe2d(nv)
    idx = np.array([0, 333, 700, 1023])
    for b in range(B):
        p = orc.lineout_params(phys, b, n_ion)
        Po, _ = orc.form_factor_2d(rng, cfg["other"]["npts"], 0.0, sa["sa"], 1, p, vx, fe2, ud_ang, va_ang, lam_index=idx)
        assert np.max(np.abs(P[b][:, idx, :] - Po) / np.abs(Po)) < 1e-7, (feature, b)


def _ff2d_check_adjoint(eng, X, fe2, Pbar, feature, ud_ang, va_ang, n_ion, gp, gf):
    """grad_phys / grad_fe2d (host) of tsff_form_factor_2d_grad for the seed Pbar: directional derivatives of <Pbar, P> by central
    differences of the HIP 2-D forward"""
    nv = fe2.shape[0]
    J = lambda Xv, f: float((eng.form_factor_2d(feature, Xv, f, ud_ang, va_ang) * Pbar).sum())
    P0 = eng.form_factor_2d(feature, X, fe2, ud_ang, va_ang)
    jabs = float((P0 * Pbar).abs().sum())
    for name in _fd_names(n_ion):
        s = util.slot_of(name)
        scale = max(abs(X[0, s]), 1e-2)

        def shifted(h, s=s):
            Xh = X.copy()
            Xh[:, s] += h
            return Xh, fe2
        err = _best_fd(J, gp[:, s].sum(), shifted, [r * scale for r in (1e-4, 1e-5, 1e-6, 1e-7)], jabs)
        assert err < 1e-4, (name, err)
    dfe = fe2 * np.cos(np.arange(nv))[None]
    an = float(np.sum(gf * dfe))
    assert _best_fd(J, an, lambda h: (X, fe2 + h * dfe), (1e-4, 1e-5, 1e-6), jabs) < 1e-4


@pytest.mark.gpu
def test_vg_loss_four_species_against_twin():
    """End to end with 4 ion species: LossFunction.vg_loss (host ravel / unravel of ThomsonParams, fraction renormalisation, Ti
    tying, the k_spectrum<4, ...> loss + gradient) against reverse-mode autodiff of the torch twin, every trainable leaf of every
    lineout in the reference's ravel order."""
    from oracle import tsadar_oracle_torch as ot
    from tsadar_amd import ThomsonParams, tree
    from tsadar_amd.loss_function import LossFunction

    B = 2
    cfg = decks.deck_fit(active=("Te", "ne", "Ti", "Z", "lam", "amp1", "Ti_same_3"), n_ion=4)
    for s, f in enumerate((0.5, 0.375, 0.25, 0.125)):   # unnormalised: renormalised by their sum (ts_params.py:543-563)
        cfg["parameters"][f"ion-{s + 1}"]["fract"]["val"] = f
    sa = util.sa_fit(B)
    batch = util.synthetic_batch(cfg, sa, B, seed=91)
    loss_fn = LossFunction(cfg, sa, batch)
    tp = ThomsonParams(cfg["parameters"], B, batch=True, activate=True)
    rng = np.random.default_rng(12)
    for k in ("Te", "Ti_2", "Z_3", "Z_4", "Ti_4"):
        tp.X[:, util.slot_of(k)] += 0.2 * rng.normal(size=B)
    diff, static = tree.partition(tp, tree.get_filter_spec(cfg["parameters"], tp))
    x0, loss_fn.unravel_weights = tree.ravel_pytree(diff)
    names = ["Te", "ne"] + [f"{k}_{s}" for s in (1, 2, 3, 4) for k in ("Ti", "Z")] + ["lam", "amp1"]
    assert x0.size == len(names) * B
    val, g = loss_fn.vg_loss(x0, static, batch)
    normed = {k: tp.X[:, util.slot_of(k)].copy() for k in orc.init_normed_params(cfg["parameters"], B, True)}
    _sensitivity_guard(cfg, sa, normed, batch, 1e-7)
    i_norm, e_norm = orc.loss_norms(cfg, batch)
    vo, ref, _, _ = ot.value_and_grad(cfg, sa, normed, batch, i_norm, e_norm, names)
    assert abs(val - vo) < 1e-9 * abs(vo), (val, vo)
    expect = np.concatenate([ref[k] for k in names])
    assert np.max(np.abs(g - expect)) <= 1e-7 * np.max(np.abs(expect)), np.max(np.abs(g - expect)) / np.max(np.abs(expect))
    assert np.all(g[names.index("Ti_3") * B:(names.index("Ti_3") + 1) * B] == 0.0)   # tied to Ti_1: no gradient of its own
