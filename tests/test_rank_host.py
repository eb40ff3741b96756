"""The host side of the exact-rank tail without a GPU.

CASES is a refusal table: every distinct fail(...) line that fake pointers can reach in the rank-tail entry points of liblaff_hip.so
(pack, similarity GEMM and its route query, the three rank_prepare forms, export, resolve, the counts, top-K, the metrics, and the
laff_rank_side checks of laff_fuse_packed_rank), plus the empty problems that return 0 before any HIP call.  These entry points look at
the context first, so the table hands them a zero-filled buffer as the context: nothing it lists gets as far as using it.  NO CALL IN
THE TABLE MAY PASS ALL ITS CHECKS -- it would launch a kernel on made-up addresses.  The expected (code, message) pairs were recorded
from the library as it was before the three rank_prepare bodies, the resolve checks and the metrics steps were each written once.
"""
import ctypes as C

import pytest
import torch

from laff_amd import _lib, ops
from laff_amd._lib import RankSide

X = C.cast(C.create_string_buffer(256), C.c_void_p)        # stands in for a laff_ctx
A, U = 0x1000, 0x1004                                      # made-up addresses: 16-byte aligned / not
OUT, ROUTE, D8 = C.byref(C.c_size_t()), C.byref(C.c_int()), (C.c_double * 8)()


def side(**fields):
    """A laff_rank_side with every pointer set, then `fields`."""
    f = dict(side=1, gt_col=A, col0=0, Ev=A, Nv=4, s_gt64=A, band=A, band_v=A, count=A, pairs=A, partials=A, tickets=A)
    f.update(fields)
    return C.byref(RankSide(**f))


# (entry point, arguments, return code, laff_last_error())
CASES = [
    ('laff_packed_bytes', (1, 1, 0, None,), -1, 'laff_packed_bytes: bad args'),
    ('laff_packed_bytes', (-1, 1, 0, OUT,), -1, 'laff_packed_bytes: bad args'),
    ('laff_packed_bytes', (1, -1, 0, OUT,), -1, 'laff_packed_bytes: bad args'),
    ('laff_packed_bytes', (1, 1, 9, OUT,), -1, 'laff_packed_bytes: bad precision 9'),
    ('laff_packed_bytes', (1, 1, -1, OUT,), -1, 'laff_packed_bytes: bad precision -1'),
    ('laff_pack_rows', (X, None, 0, 1, 4, 4, 1, 1e-13, 1.0, 1, None,), 0, ''),
    ('laff_pack_rows', (X, None, 2, 1, 4, 4, 1, 1e-13, 1.0, 1, A,), -1, 'laff_pack_rows: null E/out'),
    ('laff_pack_rows', (X, A, 2, 1, 4, 4, 1, 1e-13, 1.0, 1, None,), -1, 'laff_pack_rows: null E/out'),
    ('laff_pack_rows', (X, A, -1, 1, 4, 4, 1, 1e-13, 1.0, 1, A,), -2, 'laff_pack_rows: bad shape N=-1 H=1 d=4 lde=4'),
    ('laff_pack_rows', (X, A, 2, 0, 4, 4, 1, 1e-13, 1.0, 1, A,), -2, 'laff_pack_rows: bad shape N=2 H=0 d=4 lde=4'),
    ('laff_pack_rows', (X, A, 2, 2, 4, 7, 1, 1e-13, 1.0, 1, A,), -2, 'laff_pack_rows: bad shape N=2 H=2 d=4 lde=7'),
    ('laff_pack_rows', (X, A, 2, 1, 4, 4, 1, 1e-13, 1.0, 5, A,), -1, 'laff_pack_rows: bad precision 5'),
    ('laff_pack_rows', (X, A, 2, 1, 6, 8, 1, 1e-13, 1.0, 1, A,), -3, 'laff_pack_rows: 16-bit output needs d%4==0, lde%4==0 and 16-byte aligned buffers (d=6 lde=8)'),
    ('laff_pack_rows', (X, A, 2, 1, 4, 6, 1, 1e-13, 1.0, 3, A,), -3, 'laff_pack_rows: 16-bit output needs d%4==0, lde%4==0 and 16-byte aligned buffers (d=4 lde=6)'),
    ('laff_pack_rows', (X, U, 2, 1, 4, 4, 1, 1e-13, 1.0, 2, A,), -3, 'laff_pack_rows: 16-bit output needs d%4==0, lde%4==0 and 16-byte aligned buffers (d=4 lde=4)'),
    ('laff_pack_rows', (X, A, 2, 1, 4, 4, 1, 1e-13, 1.0, 4, U,), -3, 'laff_pack_rows: 16-bit output needs d%4==0, lde%4==0 and 16-byte aligned buffers (d=4 lde=4)'),
    ('laff_pack_rows', (None, A, 2, 1, 4, 4, 1, 1e-13, 1.0, 1, A,), -1, 'laff_pack_rows: null ctx'),
    ('laff_sim_gemm', (X, A, A, 4, 4, 8, 1.0, 1, A, 4, A, 0, None, A,), -1, 'laff_sim_gemm: gt_col needs s_gt and count'),
    ('laff_sim_gemm', (X, None, None, 0, 4, 8, 1.0, 1, None, 0, None, 0, None, None,), 0, ''),
    ('laff_sim_gemm', (X, None, None, 4, 0, 8, 1.0, 1, None, 0, None, 0, None, None,), 0, ''),
    ('laff_sim_gemm', (X, None, A, 4, 4, 8, 1.0, 1, A, 4, None, 0, None, None,), -1, 'laff_sim_gemm: null T/V'),
    ('laff_sim_gemm', (X, A, None, 4, 4, 8, 1.0, 1, A, 4, None, 0, None, None,), -1, 'laff_sim_gemm: null T/V'),
    ('laff_sim_gemm', (X, A, A, 4, 4, 8, 1.0, 5, A, 4, None, 0, None, None,), -1, 'laff_sim_gemm: bad precision 5'),
    ('laff_sim_gemm', (X, A, A, 4, 4, 8, 1.0, -1, A, 4, None, 0, None, None,), -1, 'laff_sim_gemm: bad precision -1'),
    ('laff_sim_gemm', (X, A, A, 4, 4, 0, 1.0, 0, A, 4, None, 0, None, None,), -2, 'laff_sim_gemm: K must be positive (and even for 16-bit operands) (Nt=4 Nv=4 K=0)'),
    ('laff_sim_gemm', (X, A, A, 4, 4, 7, 1.0, 1, A, 4, None, 0, None, None,), -2, 'laff_sim_gemm: K must be positive (and even for 16-bit operands) (Nt=4 Nv=4 K=7)'),
    ('laff_sim_gemm', (X, A, A, 4, 4, 7, 1.0, 4, A, 4, None, 0, None, None,), -2, 'laff_sim_gemm: K must be positive (and even for 16-bit operands) (Nt=4 Nv=4 K=7)'),
    ('laff_sim_gemm', (X, A, A, -1, 4, 8, 1.0, 1, A, 4, None, 0, None, None,), -2, 'laff_sim_gemm: K must be positive (and even for 16-bit operands) (Nt=-1 Nv=4 K=8)'),
    ('laff_sim_gemm', (X, A, A, 4, 4, 8, 1.0, 1, None, 0, None, 0, None, None,), -1, 'laff_sim_gemm: nothing to produce (S and gt_col both null)'),
    ('laff_sim_gemm', (X, A, A, 4, 4, 8, 1.0, 1, A, 2, None, 0, None, None,), -2, 'laff_sim_gemm: lds=2 < Nv=4'),
    ('laff_sim_gemm', (X, A, A, 4, 4, 8, 1.0, 1, A, 4, A, 0, A, None,), -1, 'laff_sim_gemm: gt_col needs count'),
    ('laff_sim_gemm', (X, U, A, 4, 4, 8, 1.0, 1, A, 4, None, 0, None, None,), -3, 'laff_sim_gemm: operands must be 16-byte aligned'),
    ('laff_sim_gemm', (X, A, U, 4, 4, 8, 1.0, 0, A, 4, None, 0, None, None,), -3, 'laff_sim_gemm: operands must be 16-byte aligned'),
    ('laff_sim_gemm', (None, A, A, 4, 4, 8, 1.0, 1, A, 4, None, 0, None, None,), -1, 'sim_gemm_impl: null ctx'),
    ('laff_sim_gemm_banded', (X, A, A, 4, 4, 8, 1.0, 1, A, 4, None, 0, A, A, A, A, A, 8,), -1, 'laff_sim_gemm_banded: null gt_col / s_gt64'),
    ('laff_sim_gemm_banded', (X, A, A, 4, 4, 8, 1.0, 1, A, 4, A, 0, None, A, A, A, A, 8,), -1, 'laff_sim_gemm_banded: null gt_col / s_gt64'),
    ('laff_sim_gemm_banded', (X, None, None, 0, 4, 8, 1.0, 1, None, 0, A, 0, A, None, None, None, None, 0,), 0, ''),
    ('laff_sim_gemm_banded', (X, None, A, 4, 4, 8, 1.0, 1, A, 4, A, 0, A, A, A, A, A, 8,), -1, 'laff_sim_gemm_banded: null T/V'),
    ('laff_sim_gemm_banded', (X, A, A, 4, 4, 8, 1.0, 7, A, 4, A, 0, A, A, A, A, A, 8,), -1, 'laff_sim_gemm_banded: bad precision 7'),
    ('laff_sim_gemm_banded', (X, A, A, 4, 4, 5, 1.0, 3, A, 4, A, 0, A, A, A, A, A, 8,), -2, 'laff_sim_gemm_banded: K must be positive (and even for 16-bit operands) (Nt=4 Nv=4 K=5)'),
    ('laff_sim_gemm_banded', (X, A, A, 4, 4, 8, 1.0, 1, A, 3, A, 0, A, A, A, A, A, 8,), -2, 'laff_sim_gemm_banded: lds=3 < Nv=4'),
    ('laff_sim_gemm_banded', (X, A, A, 4, 4, 8, 1.0, 1, A, 4, A, 0, A, A, A, None, A, 8,), -1, 'laff_sim_gemm_banded: gt_col needs count'),
    ('laff_sim_gemm_banded', (X, A, A, 4, 4, 8, 1.0, 1, A, 4, A, 0, A, None, A, A, A, 8,), -1, 'laff_sim_gemm_banded: the banded count needs gt_col, band_t, band_v and a pair list of >= 4 slots'),
    ('laff_sim_gemm_banded', (X, A, A, 4, 4, 8, 1.0, 1, A, 4, A, 0, A, A, None, A, A, 8,), -1, 'laff_sim_gemm_banded: the banded count needs gt_col, band_t, band_v and a pair list of >= 4 slots'),
    ('laff_sim_gemm_banded', (X, A, A, 4, 4, 8, 1.0, 1, A, 4, A, 0, A, A, A, A, None, 8,), -1, 'laff_sim_gemm_banded: the banded count needs gt_col, band_t, band_v and a pair list of >= 4 slots'),
    ('laff_sim_gemm_banded', (X, A, A, 4, 4, 8, 1.0, 1, A, 4, A, 0, A, A, A, A, A, 3,), -1, 'laff_sim_gemm_banded: the banded count needs gt_col, band_t, band_v and a pair list of >= 4 slots'),
    ('laff_sim_gemm_banded', (X, U, A, 4, 4, 8, 1.0, 1, A, 4, A, 0, A, A, A, A, A, 8,), -3, 'laff_sim_gemm_banded: operands must be 16-byte aligned'),
    ('laff_sim_gemm_banded', (X, A, A, 4, 4, 8, 1.0, 1, A, 4, U, 0, A, A, A, A, A, 8,), -3, 'laff_sim_gemm_banded: gt_col, s_gt64, band_t and band_v must be 16-byte aligned (fetched in 16-byte groups)'),
    ('laff_sim_gemm_banded', (X, A, A, 4, 4, 8, 1.0, 1, A, 4, A, 0, U + 4, A, A, A, A, 8,), -3, 'laff_sim_gemm_banded: gt_col, s_gt64, band_t and band_v must be 16-byte aligned (fetched in 16-byte groups)'),
    ('laff_sim_gemm_banded', (X, A, A, 4, 4, 8, 1.0, 1, A, 4, A, 0, A, U, A, A, A, 8,), -3, 'laff_sim_gemm_banded: gt_col, s_gt64, band_t and band_v must be 16-byte aligned (fetched in 16-byte groups)'),
    ('laff_sim_gemm_banded', (X, A, A, 4, 4, 8, 1.0, 1, None, 0, A, 0, A, A, U, A, A, 7,), -3, 'laff_sim_gemm_banded: gt_col, s_gt64, band_t and band_v must be 16-byte aligned (fetched in 16-byte groups)'),
    ('laff_sim_gemm_banded', (None, A, A, 4, 4, 8, 1.0, 1, A, 4, A, 0, A, A, A, A, A, 8,), -1, 'sim_gemm_impl: null ctx'),
    ('laff_sim_gemm_route', (X, 4, 4, 8, 1, 4, 0, 0, None,), -1, 'laff_sim_gemm_route: null route'),
    ('laff_sim_gemm_route', (X, 4, 4, 8, 5, 4, 0, 0, ROUTE,), -1, 'laff_sim_gemm_route: bad precision 5'),
    ('laff_sim_gemm_route', (X, 4, 4, 8, -1, 4, 0, 0, ROUTE,), -1, 'laff_sim_gemm_route: bad precision -1'),
    ('laff_sim_gemm_route', (X, 4, 4, 8, 1, 4, 3, 0, ROUTE,), -1, 'laff_sim_gemm_route: bad count_mode 3'),
    ('laff_sim_gemm_route', (X, 4, 4, 8, 1, 4, -1, 0, ROUTE,), -1, 'laff_sim_gemm_route: bad count_mode -1'),
    ('laff_sim_gemm_route', (X, 0, 4, 8, 1, 4, 0, 0, ROUTE,), -2, 'laff_sim_gemm_route: no launch for Nt=0 Nv=4 K=8 lds=4 count_mode=0'),
    ('laff_sim_gemm_route', (X, 4, 0, 8, 1, 4, 0, 0, ROUTE,), -2, 'laff_sim_gemm_route: no launch for Nt=4 Nv=0 K=8 lds=4 count_mode=0'),
    ('laff_sim_gemm_route', (X, 4, 4, 0, 0, 4, 0, 0, ROUTE,), -2, 'laff_sim_gemm_route: no launch for Nt=4 Nv=4 K=0 lds=4 count_mode=0'),
    ('laff_sim_gemm_route', (X, 4, 4, 7, 1, 4, 0, 0, ROUTE,), -2, 'laff_sim_gemm_route: no launch for Nt=4 Nv=4 K=7 lds=4 count_mode=0'),
    ('laff_sim_gemm_route', (X, 4, 4, 7, 4, 4, 0, 0, ROUTE,), -2, 'laff_sim_gemm_route: no launch for Nt=4 Nv=4 K=7 lds=4 count_mode=0'),
    ('laff_sim_gemm_route', (X, 4, 4, 8, 1, 3, 0, 0, ROUTE,), -2, 'laff_sim_gemm_route: no launch for Nt=4 Nv=4 K=8 lds=3 count_mode=0'),
    ('laff_sim_gemm_route', (X, 4, 4, 8, 1, 0, 0, 0, ROUTE,), -2, 'laff_sim_gemm_route: no launch for Nt=4 Nv=4 K=8 lds=0 count_mode=0'),
    ('laff_sim_gemm_route', (X, 4, 4, 8, 1, 4, 2, 3, ROUTE,), -1, 'laff_sim_gemm_route: the banded count needs a pair list of >= 4 slots'),
    ('laff_sim_gemm_route', (X, 4, 4, 8, 1, 0, 2, 0, ROUTE,), -1, 'laff_sim_gemm_route: the banded count needs a pair list of >= 4 slots'),
    ('laff_sim_gemm_route', (None, 4, 4, 8, 1, 4, 0, 0, ROUTE,), -1, 'laff_sim_gemm_route: null ctx'),
    ('laff_rank_prepare', (X, None, None, None, None, 0, 0, 1, 8, 1, 1.0, None, 0, None, None, None, None, None,), 0, ''),
    ('laff_rank_prepare', (X, None, A, A, A, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, A, A, A,), -1, 'laff_rank_prepare: null argument'),
    ('laff_rank_prepare', (X, A, A, None, A, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, A, A, A,), -1, 'laff_rank_prepare: null argument'),
    ('laff_rank_prepare', (X, A, A, A, A, 4, 4, 1, 8, 1, 1.0, None, 0, A, A, A, A, A,), -1, 'laff_rank_prepare: null argument'),
    ('laff_rank_prepare', (X, A, A, A, A, 4, 4, 1, 8, 1, 1.0, A, 0, None, A, A, A, A,), -1, 'laff_rank_prepare: null argument'),
    ('laff_rank_prepare', (X, A, A, A, A, 4, 4, 1, 8, 1, 1.0, A, 0, A, None, A, A, A,), -1, 'laff_rank_prepare: null argument'),
    ('laff_rank_prepare', (X, A, None, A, A, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, A, A, A,), -1, 'laff_rank_prepare: null argument'),
    ('laff_rank_prepare', (X, A, A, A, None, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, A, A, A,), -1, 'laff_rank_prepare: null argument'),
    ('laff_rank_prepare', (X, A, A, A, A, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, None, A, A,), -1, 'laff_rank_prepare: null argument'),
    ('laff_rank_prepare', (X, None, A, None, A, 0, 4, 1, 8, 9, 1.0, None, 0, None, None, A, None, None,), -1, 'laff_rank_prepare: bad precision 9'),
    ('laff_rank_prepare', (X, A, A, A, A, 4, 4, 1, 8, 9, 1.0, A, 0, A, A, A, A, A,), -1, 'laff_rank_prepare: bad precision 9'),
    ('laff_rank_prepare', (X, A, A, A, A, 4, 4, 1, 8, -1, 1.0, A, 0, A, A, A, A, A,), -1, 'laff_rank_prepare: bad precision -1'),
    ('laff_rank_prepare', (X, A, A, A, A, 4, 4, 1, 8, 5, 1.0, A, 0, A, A, A, A, A,), -1, 'laff_rank_prepare: bad precision 5'),
    ('laff_rank_prepare', (X, None, None, None, None, -1, 0, 1, 8, 1, 1.0, None, 0, None, None, None, None, None,), -2, 'laff_rank_prepare: need H >= 1, d % 4 == 0 (Nt=-1 Nv=0 H=1 d=8)'),
    ('laff_rank_prepare', (X, None, None, None, None, 0, -1, 1, 8, 1, 1.0, None, 0, None, None, None, None, None,), -2, 'laff_rank_prepare: need H >= 1, d % 4 == 0 (Nt=0 Nv=-1 H=1 d=8)'),
    ('laff_rank_prepare', (X, A, A, A, A, 4, 4, 0, 8, 1, 1.0, A, 0, A, A, A, A, A,), -2, 'laff_rank_prepare: need H >= 1, d % 4 == 0 (Nt=4 Nv=4 H=0 d=8)'),
    ('laff_rank_prepare', (X, A, A, A, A, 4, 4, 1, 0, 1, 1.0, A, 0, A, A, A, A, A,), -2, 'laff_rank_prepare: need H >= 1, d % 4 == 0 (Nt=4 Nv=4 H=1 d=0)'),
    ('laff_rank_prepare', (X, A, A, A, A, 4, 4, 2, 6, 3, 1.0, A, 0, A, A, A, A, A,), -2, 'laff_rank_prepare: need H >= 1, d % 4 == 0 (Nt=4 Nv=4 H=2 d=6)'),
    ('laff_rank_prepare', (X, A, A, A, A, 4, 4, 1, 8, 1, 0.0, A, 0, A, A, A, A, A,), -1, 'laff_rank_prepare: prescale must be positive'),
    ('laff_rank_prepare', (X, A, A, A, A, 4, 4, 1, 8, 1, -2.0, A, 0, A, A, A, A, A,), -1, 'laff_rank_prepare: prescale must be positive'),
    ('laff_rank_prepare', (X, A, A, A, A, 4, 4, 1, 8, 1, float("nan"), A, 0, A, A, A, A, A,), -1, 'laff_rank_prepare: prescale must be positive'),
    ('laff_rank_prepare', (X, U, A, A, A, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, A, A, A,), -3, 'laff_rank_prepare: embeddings and operands must be 16-byte aligned'),
    ('laff_rank_prepare', (X, A, U, A, A, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, A, A, A,), -3, 'laff_rank_prepare: embeddings and operands must be 16-byte aligned'),
    ('laff_rank_prepare', (X, A, A, U, A, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, A, A, A,), -3, 'laff_rank_prepare: embeddings and operands must be 16-byte aligned'),
    ('laff_rank_prepare', (X, A, A, A, U, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, A, A, A,), -3, 'laff_rank_prepare: embeddings and operands must be 16-byte aligned'),
    ('laff_rank_prepare', (X, None, U, None, A, 0, 4, 1, 8, 1, 1.0, None, 0, None, None, A, None, None,), -3, 'laff_rank_prepare: embeddings and operands must be 16-byte aligned'),
    ('laff_rank_prepare', (None, A, A, A, A, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, A, A, A,), -1, 'laff_rank_prepare: null ctx'),
    ('laff_rank_prepare_part', (X, 0, A, A, A, A, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, A, A, A,), -1, 'laff_rank_prepare_part: sides must be 1 (text rows) or 2 (video rows)'),
    ('laff_rank_prepare_part', (X, 3, A, A, A, A, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, A, A, A,), -1, 'laff_rank_prepare_part: sides must be 1 (text rows) or 2 (video rows)'),
    ('laff_rank_prepare_part', (X, -1, A, A, A, A, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, A, A, A,), -1, 'laff_rank_prepare_part: sides must be 1 (text rows) or 2 (video rows)'),
    ('laff_rank_prepare_part', (X, 1, None, None, None, None, 0, 4, 1, 8, 1, 1.0, None, 0, None, None, None, None, None,), 0, ''),
    ('laff_rank_prepare_part', (X, 2, None, None, None, None, 4, 0, 1, 8, 1, 1.0, None, 0, None, None, None, None, None,), 0, ''),
    ('laff_rank_prepare_part', (X, 1, None, A, A, None, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, None, None, None,), -1, 'laff_rank_prepare_part: null argument (text side)'),
    ('laff_rank_prepare_part', (X, 1, A, None, A, None, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, None, None, None,), -1, 'laff_rank_prepare_part: null argument (text side)'),
    ('laff_rank_prepare_part', (X, 1, A, A, None, None, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, None, None, None,), -1, 'laff_rank_prepare_part: null argument (text side)'),
    ('laff_rank_prepare_part', (X, 1, A, A, A, None, 4, 4, 1, 8, 1, 1.0, None, 0, A, A, None, None, None,), -1, 'laff_rank_prepare_part: null argument (text side)'),
    ('laff_rank_prepare_part', (X, 1, A, A, A, None, 4, 4, 1, 8, 1, 1.0, A, 0, None, A, None, None, None,), -1, 'laff_rank_prepare_part: null argument (text side)'),
    ('laff_rank_prepare_part', (X, 1, A, A, A, None, 4, 4, 1, 8, 1, 1.0, A, 0, A, None, None, None, None,), -1, 'laff_rank_prepare_part: null argument (text side)'),
    ('laff_rank_prepare_part', (X, 2, None, None, None, A, 0, 4, 1, 8, 1, 1.0, None, 0, None, None, A, None, None,), -1, 'laff_rank_prepare_part: null argument (video side)'),
    ('laff_rank_prepare_part', (X, 2, None, A, None, None, 0, 4, 1, 8, 1, 1.0, None, 0, None, None, A, None, None,), -1, 'laff_rank_prepare_part: null argument (video side)'),
    ('laff_rank_prepare_part', (X, 2, None, A, None, A, 0, 4, 1, 8, 1, 1.0, None, 0, None, None, None, None, None,), -1, 'laff_rank_prepare_part: null argument (video side)'),
    ('laff_rank_prepare_part', (X, 1, A, None, A, None, 4, 0, 1, 8, 9, 1.0, A, 0, A, A, None, None, None,), -1, 'laff_rank_prepare_part: bad precision 9'),
    ('laff_rank_prepare_part', (X, 2, None, A, None, A, 0, 4, 1, 8, -1, 1.0, None, 0, None, None, A, None, None,), -1, 'laff_rank_prepare_part: bad precision -1'),
    ('laff_rank_prepare_part', (X, 1, A, A, A, None, 4, 4, 0, 8, 1, 1.0, A, 0, A, A, None, None, None,), -2, 'laff_rank_prepare_part: need H >= 1, d % 4 == 0 (Nt=4 Nv=4 H=0 d=8)'),
    ('laff_rank_prepare_part', (X, 1, A, A, A, None, 4, -1, 1, 8, 1, 1.0, A, 0, A, A, None, None, None,), -2, 'laff_rank_prepare_part: need H >= 1, d % 4 == 0 (Nt=4 Nv=-1 H=1 d=8)'),
    ('laff_rank_prepare_part', (X, 2, None, A, None, A, -1, 4, 1, 8, 1, 1.0, None, 0, None, None, A, None, None,), -2, 'laff_rank_prepare_part: need H >= 1, d % 4 == 0 (Nt=-1 Nv=4 H=1 d=8)'),
    ('laff_rank_prepare_part', (X, 2, None, A, None, A, 0, 4, 1, 10, 1, 1.0, None, 0, None, None, A, None, None,), -2, 'laff_rank_prepare_part: need H >= 1, d % 4 == 0 (Nt=0 Nv=4 H=1 d=10)'),
    ('laff_rank_prepare_part', (X, 1, A, A, A, None, 4, 4, 1, 8, 1, 0.0, A, 0, A, A, None, None, None,), -1, 'laff_rank_prepare_part: prescale must be positive'),
    ('laff_rank_prepare_part', (X, 2, None, A, None, A, 0, 4, 1, 8, 1, -1.0, None, 0, None, None, A, None, None,), -1, 'laff_rank_prepare_part: prescale must be positive'),
    ('laff_rank_prepare_part', (X, 1, U, A, A, None, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, None, None, None,), -3, 'laff_rank_prepare_part: embeddings and operands must be 16-byte aligned'),
    ('laff_rank_prepare_part', (X, 1, A, U, A, None, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, None, None, None,), -3, 'laff_rank_prepare_part: embeddings and operands must be 16-byte aligned'),
    ('laff_rank_prepare_part', (X, 1, A, A, U, None, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, None, None, None,), -3, 'laff_rank_prepare_part: embeddings and operands must be 16-byte aligned'),
    ('laff_rank_prepare_part', (X, 1, A, A, A, U, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, None, None, None,), -3, 'laff_rank_prepare_part: embeddings and operands must be 16-byte aligned'),
    ('laff_rank_prepare_part', (X, 2, U, A, None, A, 0, 4, 1, 8, 1, 1.0, None, 0, None, None, A, None, None,), -3, 'laff_rank_prepare_part: embeddings and operands must be 16-byte aligned'),
    ('laff_rank_prepare_part', (X, 2, None, A, None, U, 0, 4, 1, 8, 1, 1.0, None, 0, None, None, A, None, None,), -3, 'laff_rank_prepare_part: embeddings and operands must be 16-byte aligned'),
    ('laff_rank_prepare_part', (None, 1, A, A, A, None, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, None, None, None,), -1, 'laff_rank_prepare_part: null ctx'),
    ('laff_rank_prepare_emit', (X, 0, A, A, A, A, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, A, A, A,), -1, 'laff_rank_prepare_emit: emit must be 1 (T), 2 (V) or 3 (both)'),
    ('laff_rank_prepare_emit', (X, 4, A, A, A, A, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, A, A, A,), -1, 'laff_rank_prepare_emit: emit must be 1 (T), 2 (V) or 3 (both)'),
    ('laff_rank_prepare_emit', (X, -1, A, A, A, A, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, A, A, A,), -1, 'laff_rank_prepare_emit: emit must be 1 (T), 2 (V) or 3 (both)'),
    ('laff_rank_prepare_emit', (X, 3, A, A, A, A, 4, 4, 1, 8, 0, 1.0, A, 0, A, A, A, A, A,), -5, 'laff_rank_prepare_emit: single-plane 16-bit operands only (precision 0): call laff_pack_rows + laff_rank_prepare'),
    ('laff_rank_prepare_emit', (X, 3, A, A, A, A, 4, 4, 1, 8, 3, 1.0, A, 0, A, A, A, A, A,), -5, 'laff_rank_prepare_emit: single-plane 16-bit operands only (precision 3): call laff_pack_rows + laff_rank_prepare'),
    ('laff_rank_prepare_emit', (X, 3, A, A, A, A, 4, 4, 1, 8, 4, 1.0, A, 0, A, A, A, A, A,), -5, 'laff_rank_prepare_emit: single-plane 16-bit operands only (precision 4): call laff_pack_rows + laff_rank_prepare'),
    ('laff_rank_prepare_emit', (X, 3, A, A, A, A, 4, 4, 1, 8, 9, 1.0, A, 0, A, A, A, A, A,), -5, 'laff_rank_prepare_emit: single-plane 16-bit operands only (precision 9): call laff_pack_rows + laff_rank_prepare'),
    ('laff_rank_prepare_emit', (X, 3, A, A, A, A, 4, 4, 1, 8, -1, 1.0, A, 0, A, A, A, A, A,), -5, 'laff_rank_prepare_emit: single-plane 16-bit operands only (precision -1): call laff_pack_rows + laff_rank_prepare'),
    ('laff_rank_prepare_emit', (X, 3, None, None, None, None, 0, 4, 1, 8, 1, 1.0, None, 0, None, None, None, None, None,), 0, ''),
    ('laff_rank_prepare_emit', (X, 1, None, None, None, None, 4, 0, 1, 8, 2, 1.0, None, 0, None, None, None, None, None,), 0, ''),
    ('laff_rank_prepare_emit', (X, 3, None, A, A, A, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, A, A, A,), -1, 'laff_rank_prepare_emit: null argument'),
    ('laff_rank_prepare_emit', (X, 3, A, None, A, A, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, A, A, A,), -1, 'laff_rank_prepare_emit: null argument'),
    ('laff_rank_prepare_emit', (X, 3, A, A, None, A, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, A, A, A,), -1, 'laff_rank_prepare_emit: null argument'),
    ('laff_rank_prepare_emit', (X, 3, A, A, A, None, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, A, A, A,), -1, 'laff_rank_prepare_emit: null argument'),
    ('laff_rank_prepare_emit', (X, 3, A, A, A, A, 4, 4, 1, 8, 1, 1.0, None, 0, A, A, A, A, A,), -1, 'laff_rank_prepare_emit: null argument'),
    ('laff_rank_prepare_emit', (X, 3, A, A, A, A, 4, 4, 1, 8, 1, 1.0, A, 0, None, A, A, A, A,), -1, 'laff_rank_prepare_emit: null argument'),
    ('laff_rank_prepare_emit', (X, 3, A, A, A, A, 4, 4, 1, 8, 1, 1.0, A, 0, A, None, A, A, A,), -1, 'laff_rank_prepare_emit: null argument'),
    ('laff_rank_prepare_emit', (X, 3, A, A, A, A, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, None, A, A,), -1, 'laff_rank_prepare_emit: null argument'),
    ('laff_rank_prepare_emit', (X, 3, A, A, A, A, -1, 4, 1, 8, 1, 1.0, A, 0, A, A, A, A, A,), -2, 'laff_rank_prepare_emit: need H >= 1, d % 4 == 0 (Nt=-1 Nv=4 H=1 d=8)'),
    ('laff_rank_prepare_emit', (X, 3, A, A, A, A, 4, 4, 0, 8, 2, 1.0, A, 0, A, A, A, A, A,), -2, 'laff_rank_prepare_emit: need H >= 1, d % 4 == 0 (Nt=4 Nv=4 H=0 d=8)'),
    ('laff_rank_prepare_emit', (X, 2, A, A, A, A, 4, 4, 1, 6, 1, 1.0, A, 0, A, A, A, A, A,), -2, 'laff_rank_prepare_emit: need H >= 1, d % 4 == 0 (Nt=4 Nv=4 H=1 d=6)'),
    ('laff_rank_prepare_emit', (X, 3, A, A, A, A, 4, 4, 1, 8, 1, 0.0, A, 0, A, A, A, A, A,), -1, 'laff_rank_prepare_emit: prescale must be positive'),
    ('laff_rank_prepare_emit', (X, 3, U, A, A, A, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, A, A, A,), -3, 'laff_rank_prepare_emit: embeddings and operands must be 16-byte aligned'),
    ('laff_rank_prepare_emit', (X, 3, A, U, A, A, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, A, A, A,), -3, 'laff_rank_prepare_emit: embeddings and operands must be 16-byte aligned'),
    ('laff_rank_prepare_emit', (X, 3, A, A, U, A, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, A, A, A,), -3, 'laff_rank_prepare_emit: embeddings and operands must be 16-byte aligned'),
    ('laff_rank_prepare_emit', (X, 3, A, A, A, U, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, A, A, A,), -3, 'laff_rank_prepare_emit: embeddings and operands must be 16-byte aligned'),
    ('laff_rank_prepare_emit', (None, 3, A, A, A, A, 4, 4, 1, 8, 1, 1.0, A, 0, A, A, A, A, A,), -1, 'laff_rank_prepare_emit: null ctx'),
    ('laff_rank_export_pairs', (X, None, A, None, 0, 4, A, 8, A, 2, 0, A, 8, A,), -1, 'laff_rank_export_pairs: null argument'),
    ('laff_rank_export_pairs', (X, A, None, None, 0, 4, A, 8, A, 2, 0, A, 8, A,), -1, 'laff_rank_export_pairs: null argument'),
    ('laff_rank_export_pairs', (X, A, A, None, 0, 4, None, 8, A, 2, 0, A, 8, A,), -1, 'laff_rank_export_pairs: null argument'),
    ('laff_rank_export_pairs', (X, A, A, None, 0, 4, A, 8, None, 2, 0, A, 8, A,), -1, 'laff_rank_export_pairs: null argument'),
    ('laff_rank_export_pairs', (X, A, A, None, 0, 4, A, 8, A, 2, 0, None, 8, A,), -1, 'laff_rank_export_pairs: null argument'),
    ('laff_rank_export_pairs', (X, A, A, None, 0, 4, A, 8, A, 2, 0, A, 8, None,), -1, 'laff_rank_export_pairs: null argument'),
    ('laff_rank_export_pairs', (X, A, A, None, 0, 4, A, 8, A, 0, 0, A, 8, A,), -2, 'laff_rank_export_pairs: need 1 <= world <= 16, cap % 4 == 0 (world=0 cap=8)'),
    ('laff_rank_export_pairs', (X, A, A, None, 0, 4, A, 8, A, 17, 0, A, 8, A,), -2, 'laff_rank_export_pairs: need 1 <= world <= 16, cap % 4 == 0 (world=17 cap=8)'),
    ('laff_rank_export_pairs', (X, A, A, None, 0, 4, A, 8, A, 2, 0, A, 3, A,), -2, 'laff_rank_export_pairs: need 1 <= world <= 16, cap % 4 == 0 (world=2 cap=3)'),
    ('laff_rank_export_pairs', (X, A, A, None, 0, 4, A, 8, A, 2, 0, A, 6, A,), -2, 'laff_rank_export_pairs: need 1 <= world <= 16, cap % 4 == 0 (world=2 cap=6)'),
    ('laff_rank_export_pairs', (X, A, A, None, 0, 4, A, 3, A, 2, 0, A, 8, A,), -2, 'laff_rank_export_pairs: need 1 <= world <= 16, cap % 4 == 0 (world=2 cap=8)'),
    ('laff_rank_export_pairs', (X, A, A, A, 3, 4, A, 8, A, 2, 0, A, 8, A,), -2, 'laff_rank_export_pairs: lds=3 < Nv=4'),
    ('laff_rank_export_pairs', (X, A, A, None, 0, 4, A, 8, A, 2, 0, U, 8, A,), -3, 'laff_rank_export_pairs: out must be 16-byte aligned'),
    ('laff_rank_export_pairs', (None, A, A, None, 0, 4, A, 8, A, 2, 0, A, 8, A,), -1, 'laff_rank_export_pairs: null ctx'),
    ('laff_rank_resolve', (X, None, None, 0, 4, 1, 8, None, None, None, 0, None, 0,), 0, ''),
    ('laff_rank_resolve', (X, None, None, 4, 0, 1, 8, None, None, None, 0, None, 0,), 0, ''),
    ('laff_rank_resolve', (X, None, A, 4, 4, 1, 8, A, A, None, 0, A, 8,), -1, 'laff_rank_resolve: null argument'),
    ('laff_rank_resolve', (X, A, None, 4, 4, 1, 8, A, A, None, 0, A, 8,), -1, 'laff_rank_resolve: null argument'),
    ('laff_rank_resolve', (X, A, A, 4, 4, 1, 8, None, A, None, 0, A, 8,), -1, 'laff_rank_resolve: null argument'),
    ('laff_rank_resolve', (X, A, A, 4, 4, 1, 8, A, None, None, 0, A, 8,), -1, 'laff_rank_resolve: null argument'),
    ('laff_rank_resolve', (X, A, A, 4, 4, 1, 8, A, A, None, 0, None, 8,), -1, 'laff_rank_resolve: null argument'),
    ('laff_rank_resolve', (X, A, A, -1, 4, 1, 8, A, A, None, 0, A, 8,), -2, 'laff_rank_resolve: bad shape'),
    ('laff_rank_resolve', (X, A, A, 4, -1, 1, 8, A, A, None, 0, A, 8,), -2, 'laff_rank_resolve: bad shape'),
    ('laff_rank_resolve', (X, A, A, 4, 4, 0, 8, A, A, None, 0, A, 8,), -2, 'laff_rank_resolve: bad shape'),
    ('laff_rank_resolve', (X, A, A, 4, 4, 1, 0, A, A, None, 0, A, 8,), -2, 'laff_rank_resolve: bad shape'),
    ('laff_rank_resolve', (X, A, A, 4, 4, 1, 6, A, A, None, 0, A, 8,), -2, 'laff_rank_resolve: bad shape'),
    ('laff_rank_resolve', (X, A, A, 4, 4, 1, 8, A, A, None, 0, A, 3,), -2, 'laff_rank_resolve: bad shape'),
    ('laff_rank_resolve', (X, A, A, 4, 4, 1, 8, A, A, None, 0, A, 0,), -2, 'laff_rank_resolve: bad shape'),
    ('laff_rank_resolve', (X, A, A, 4, 4, 1, 8, A, A, A, 2, A, 8,), -2, 'laff_rank_resolve: lds=2 < Nv=4'),
    ('laff_rank_resolve', (X, U, A, 4, 4, 1, 8, A, A, None, 0, A, 8,), -3, 'laff_rank_resolve: embeddings must be 16-byte aligned'),
    ('laff_rank_resolve', (X, A, U, 4, 4, 1, 8, A, A, A, 4, A, 7,), -3, 'laff_rank_resolve: embeddings must be 16-byte aligned'),
    ('laff_rank_resolve', (None, A, A, 4, 4, 1, 8, A, A, None, 0, A, 8,), -1, 'laff_rank_resolve: null ctx'),
    ('laff_rank_resolve_metrics', (X, A, A, 4, 4, 1, 8, A, A, None, 0, A, 8, 1, None, None, 1,), -1, 'laff_rank_resolve_metrics: null out8'),
    ('laff_rank_resolve_metrics', (X, A, A, 0, 4, 1, 8, A, A, None, 0, A, 8, 1, None, D8, 1,), -2, 'laff_rank_resolve_metrics: Nt=0 Nv=4 (the metrics of an empty query set are undefined)'),
    ('laff_rank_resolve_metrics', (X, A, A, 4, 0, 1, 8, A, A, None, 0, A, 8, 1, None, D8, 1,), -2, 'laff_rank_resolve_metrics: Nt=4 Nv=0 (the metrics of an empty query set are undefined)'),
    ('laff_rank_resolve_metrics', (X, A, A, -1, 4, 1, 8, A, A, None, 0, A, 8, 1, None, D8, 1,), -2, 'laff_rank_resolve_metrics: Nt=-1 Nv=4 (the metrics of an empty query set are undefined)'),
    ('laff_rank_resolve_metrics', (X, A, A, 4, -3, 1, 8, A, A, None, 0, A, 8, 1, None, D8, 1,), -2, 'laff_rank_resolve_metrics: Nt=4 Nv=-3 (the metrics of an empty query set are undefined)'),
    ('laff_rank_resolve_metrics', (X, None, A, 4, 4, 1, 8, A, A, None, 0, A, 8, 1, None, D8, 0,), -1, 'laff_rank_resolve_metrics: null argument'),
    ('laff_rank_resolve_metrics', (X, A, None, 4, 4, 1, 8, A, A, None, 0, A, 8, 1, None, D8, 0,), -1, 'laff_rank_resolve_metrics: null argument'),
    ('laff_rank_resolve_metrics', (X, A, A, 4, 4, 1, 8, None, A, None, 0, A, 8, 1, None, D8, 0,), -1, 'laff_rank_resolve_metrics: null argument'),
    ('laff_rank_resolve_metrics', (X, A, A, 4, 4, 1, 8, A, None, None, 0, A, 8, 1, None, D8, 0,), -1, 'laff_rank_resolve_metrics: null argument'),
    ('laff_rank_resolve_metrics', (X, A, A, 4, 4, 1, 8, A, A, None, 0, None, 8, 1, None, D8, 0,), -1, 'laff_rank_resolve_metrics: null argument'),
    ('laff_rank_resolve_metrics', (X, A, A, 4, 4, 0, 8, A, A, None, 0, A, 8, 1, None, D8, 1,), -2, 'laff_rank_resolve_metrics: bad shape'),
    ('laff_rank_resolve_metrics', (X, A, A, 4, 4, 1, 0, A, A, None, 0, A, 8, 1, None, D8, 1,), -2, 'laff_rank_resolve_metrics: bad shape'),
    ('laff_rank_resolve_metrics', (X, A, A, 4, 4, 1, 6, A, A, None, 0, A, 8, 1, None, D8, 1,), -2, 'laff_rank_resolve_metrics: bad shape'),
    ('laff_rank_resolve_metrics', (X, A, A, 4, 4, 1, 8, A, A, None, 0, A, 3, 1, None, D8, 1,), -2, 'laff_rank_resolve_metrics: bad shape'),
    ('laff_rank_resolve_metrics', (X, A, A, 4, 4, 1, 8, A, A, None, 0, A, 0, 1, None, D8, 1,), -2, 'laff_rank_resolve_metrics: bad shape'),
    ('laff_rank_resolve_metrics', (X, A, A, 4, 4, 1, 8, A, A, A, 2, A, 8, 1, None, D8, 1,), -2, 'laff_rank_resolve_metrics: lds=2 < Nv=4'),
    ('laff_rank_resolve_metrics', (X, U, A, 4, 4, 1, 8, A, A, None, 0, A, 8, 1, None, D8, 0,), -3, 'laff_rank_resolve_metrics: embeddings must be 16-byte aligned'),
    ('laff_rank_resolve_metrics', (X, A, U, 4, 4, 1, 8, A, A, A, 4, A, 7, 1, A, D8, 1,), -3, 'laff_rank_resolve_metrics: embeddings must be 16-byte aligned'),
    ('laff_rank_resolve_metrics', (None, A, A, 4, 4, 1, 8, A, A, None, 0, A, 8, 1, None, D8, 1,), -1, 'laff_rank_resolve_metrics: null ctx'),
    ('laff_gather_gt', (X, None, 0, 4, 4, None, 0, None,), 0, ''),
    ('laff_gather_gt', (X, None, 4, 4, 4, A, 0, A,), -1, 'laff_gather_gt: null argument'),
    ('laff_gather_gt', (X, A, 4, 4, 4, None, 0, A,), -1, 'laff_gather_gt: null argument'),
    ('laff_gather_gt', (X, A, 4, 4, 4, A, 0, None,), -1, 'laff_gather_gt: null argument'),
    ('laff_gather_gt', (X, A, -1, 4, 4, A, 0, A,), -2, 'laff_gather_gt: bad shape'),
    ('laff_gather_gt', (X, A, 4, -1, 4, A, 0, A,), -2, 'laff_gather_gt: bad shape'),
    ('laff_gather_gt', (X, A, 4, 4, 3, A, 0, A,), -2, 'laff_gather_gt: bad shape'),
    ('laff_gather_gt', (None, A, 4, 4, 4, A, 0, A,), -1, 'laff_gather_gt: null ctx'),
    ('laff_rank_count', (X, None, 0, 4, 4, None, 0, None, None, 0,), 0, ''),
    ('laff_rank_count', (X, None, 4, 4, 4, A, 0, A, A, 0,), -1, 'laff_rank_count: null argument'),
    ('laff_rank_count', (X, A, 4, 4, 4, None, 0, A, A, 0,), -1, 'laff_rank_count: null argument'),
    ('laff_rank_count', (X, A, 4, 4, 4, A, 0, None, A, 0,), -1, 'laff_rank_count: null argument'),
    ('laff_rank_count', (X, A, 4, 4, 4, A, 0, A, None, 0,), -1, 'laff_rank_count: null argument'),
    ('laff_rank_count', (X, A, -1, 4, 4, A, 0, A, A, 1,), -2, 'laff_rank_count: bad shape'),
    ('laff_rank_count', (X, A, 4, -1, 4, A, 0, A, A, 1,), -2, 'laff_rank_count: bad shape'),
    ('laff_rank_count', (X, A, 4, 4, 3, A, 0, A, A, 1,), -2, 'laff_rank_count: bad shape'),
    ('laff_rank_count', (None, A, 4, 4, 4, A, 0, A, A, 0,), -1, 'laff_rank_count: null ctx'),
    ('laff_topk_rows', (X, None, 0, 4, 4, 2, None, None,), 0, ''),
    ('laff_topk_rows', (X, None, 4, 4, 4, 2, A, A,), -1, 'laff_topk_rows: null argument'),
    ('laff_topk_rows', (X, A, 4, 4, 4, 2, None, A,), -1, 'laff_topk_rows: null argument'),
    ('laff_topk_rows', (X, A, 4, 4, 4, 2, A, None,), -1, 'laff_topk_rows: null argument'),
    ('laff_topk_rows', (X, A, -1, 4, 4, 2, A, A,), -2, 'laff_topk_rows: need 1 <= K <= min(Nv, 8192) (Nt=-1 Nv=4 K=2)'),
    ('laff_topk_rows', (X, A, 4, 0, 4, 1, A, A,), -2, 'laff_topk_rows: need 1 <= K <= min(Nv, 8192) (Nt=4 Nv=0 K=1)'),
    ('laff_topk_rows', (X, A, 4, 4, 3, 2, A, A,), -2, 'laff_topk_rows: need 1 <= K <= min(Nv, 8192) (Nt=4 Nv=4 K=2)'),
    ('laff_topk_rows', (X, A, 4, 4, 4, 0, A, A,), -2, 'laff_topk_rows: need 1 <= K <= min(Nv, 8192) (Nt=4 Nv=4 K=0)'),
    ('laff_topk_rows', (X, A, 4, 4, 4, 5, A, A,), -2, 'laff_topk_rows: need 1 <= K <= min(Nv, 8192) (Nt=4 Nv=4 K=5)'),
    ('laff_topk_rows', (X, A, 4, 9000, 9000, 8193, A, A,), -2, 'laff_topk_rows: need 1 <= K <= min(Nv, 8192) (Nt=4 Nv=9000 K=8193)'),
    ('laff_topk_rows', (X, A, 4, 100000, 100000, 64, A, A,), -5, 'laff_topk_rows: Nv=100000 with K=64 does not fit the LDS-resident row (40572 columns at most: split the columns and merge the per-block lists, as laff_amd.ops.topk_rows does)'),
    ('laff_topk_rows', (X, A, 4, 40000, 40000, 65, A, A,), -5, 'laff_topk_rows: Nv=40000 with K=65 does not fit the LDS-resident row (39676 columns at most: split the columns and merge the per-block lists, as laff_amd.ops.topk_rows does)'),
    ('laff_topk_rows', (X, A, 4, 30000, 30000, 8192, A, A,), -5, 'laff_topk_rows: Nv=30000 with K=8192 does not fit the LDS-resident row (24316 columns at most: split the columns and merge the per-block lists, as laff_amd.ops.topk_rows does)'),
    ('laff_topk_rows', (X, A, 4, 40704, 40704, 64, A, A,), -5, 'laff_topk_rows: Nv=40704 with K=64 does not fit the LDS-resident row (40572 columns at most: split the columns and merge the per-block lists, as laff_amd.ops.topk_rows does)'),
    ('laff_topk_rows', (None, A, 4, 4, 4, 2, A, A,), -1, 'laff_topk_rows: null ctx'),
    ('laff_v2t_count', (X, None, 0, 4, 4, None, None, 2, None,), 0, ''),
    ('laff_v2t_count', (X, None, 4, 0, 4, None, None, 2, None,), 0, ''),
    ('laff_v2t_count', (X, A, 4, 4, 4, A, A, 0, A,), 0, ''),
    ('laff_v2t_count', (X, None, 4, 4, 4, A, A, 2, A,), -1, 'laff_v2t_count: null argument'),
    ('laff_v2t_count', (X, A, 4, 4, 4, None, A, 2, A,), -1, 'laff_v2t_count: null argument'),
    ('laff_v2t_count', (X, A, 4, 4, 4, A, None, 2, A,), -1, 'laff_v2t_count: null argument'),
    ('laff_v2t_count', (X, A, 4, 4, 4, A, A, 2, None,), -1, 'laff_v2t_count: null argument'),
    ('laff_v2t_count', (X, A, -1, 4, 4, A, A, 2, A,), -2, 'laff_v2t_count: bad shape'),
    ('laff_v2t_count', (X, A, 4, -1, 4, A, A, 2, A,), -2, 'laff_v2t_count: bad shape'),
    ('laff_v2t_count', (X, A, 4, 4, 3, A, A, 2, A,), -2, 'laff_v2t_count: bad shape'),
    ('laff_v2t_count', (X, A, 4, 4, 4, A, A, -1, A,), -2, 'laff_v2t_count: bad shape'),
    ('laff_v2t_count', (None, A, 4, 4, 4, A, A, 2, A,), -1, 'laff_v2t_count: null ctx'),
    ('laff_v2t_count_exact', (X, None, 0, 4, 4, None, None, 2, None, None, 1, 8, None, None, None, None, None, 0,), 0, ''),
    ('laff_v2t_count_exact', (X, None, 4, 0, 4, None, None, 2, None, None, 1, 8, None, None, None, None, None, 0,), 0, ''),
    ('laff_v2t_count_exact', (X, None, 4, 4, 4, A, A, 2, A, A, 1, 8, A, A, A, A, A, 16,), -1, 'laff_v2t_count_exact: null argument'),
    ('laff_v2t_count_exact', (X, A, 4, 4, 4, None, A, 2, A, A, 1, 8, A, A, A, A, A, 16,), -1, 'laff_v2t_count_exact: null argument'),
    ('laff_v2t_count_exact', (X, A, 4, 4, 4, A, None, 2, A, A, 1, 8, A, A, A, A, A, 16,), -1, 'laff_v2t_count_exact: null argument'),
    ('laff_v2t_count_exact', (X, A, 4, 4, 4, A, A, 2, None, A, 1, 8, A, A, A, A, A, 16,), -1, 'laff_v2t_count_exact: null argument'),
    ('laff_v2t_count_exact', (X, A, 4, 4, 4, A, A, 2, A, None, 1, 8, A, A, A, A, A, 16,), -1, 'laff_v2t_count_exact: null argument'),
    ('laff_v2t_count_exact', (X, A, 4, 4, 4, A, A, 2, A, A, 1, 8, None, A, A, A, A, 16,), -1, 'laff_v2t_count_exact: null argument'),
    ('laff_v2t_count_exact', (X, A, 4, 4, 4, A, A, 2, A, A, 1, 8, A, None, A, A, A, 16,), -1, 'laff_v2t_count_exact: null argument'),
    ('laff_v2t_count_exact', (X, A, 4, 4, 4, A, A, 2, A, A, 1, 8, A, A, None, A, A, 16,), -1, 'laff_v2t_count_exact: null argument'),
    ('laff_v2t_count_exact', (X, A, 4, 4, 4, A, A, 2, A, A, 1, 8, A, A, A, None, A, 16,), -1, 'laff_v2t_count_exact: null argument'),
    ('laff_v2t_count_exact', (X, A, 4, 4, 4, A, A, 2, A, A, 1, 8, A, A, A, A, None, 16,), -1, 'laff_v2t_count_exact: null argument'),
    ('laff_v2t_count_exact', (X, A, -1, 4, 4, A, A, 2, A, A, 1, 8, A, A, A, A, A, 16,), -2, 'laff_v2t_count_exact: bad shape (Nt=-1 Nv=4 lds=4 H=1 d=8: d must be a multiple of 4)'),
    ('laff_v2t_count_exact', (X, A, 4, -1, 4, A, A, 2, A, A, 1, 8, A, A, A, A, A, 16,), -2, 'laff_v2t_count_exact: bad shape (Nt=4 Nv=-1 lds=4 H=1 d=8: d must be a multiple of 4)'),
    ('laff_v2t_count_exact', (X, A, 4, 4, 3, A, A, 2, A, A, 1, 8, A, A, A, A, A, 16,), -2, 'laff_v2t_count_exact: bad shape (Nt=4 Nv=4 lds=3 H=1 d=8: d must be a multiple of 4)'),
    ('laff_v2t_count_exact', (X, A, 4, 4, 4, A, A, -1, A, A, 1, 8, A, A, A, A, A, 16,), -2, 'laff_v2t_count_exact: bad shape (Nt=4 Nv=4 lds=4 H=1 d=8: d must be a multiple of 4)'),
    ('laff_v2t_count_exact', (X, A, 4, 4, 4, A, A, 2, A, A, 0, 8, A, A, A, A, A, 16,), -2, 'laff_v2t_count_exact: bad shape (Nt=4 Nv=4 lds=4 H=0 d=8: d must be a multiple of 4)'),
    ('laff_v2t_count_exact', (X, A, 4, 4, 4, A, A, 2, A, A, 1, 0, A, A, A, A, A, 16,), -2, 'laff_v2t_count_exact: bad shape (Nt=4 Nv=4 lds=4 H=1 d=0: d must be a multiple of 4)'),
    ('laff_v2t_count_exact', (X, A, 4, 4, 4, A, A, 2, A, A, 1, 6, A, A, A, A, A, 16,), -2, 'laff_v2t_count_exact: bad shape (Nt=4 Nv=4 lds=4 H=1 d=6: d must be a multiple of 4)'),
    ('laff_v2t_count_exact', (X, A, 4, 4, 4, A, A, 2, U, A, 1, 8, A, A, A, A, A, 16,), -3, 'laff_v2t_count_exact: embeddings must be 16-byte aligned'),
    ('laff_v2t_count_exact', (X, A, 4, 4, 4, A, A, 2, A, U, 1, 8, A, A, A, A, A, 16,), -3, 'laff_v2t_count_exact: embeddings must be 16-byte aligned'),
    ('laff_v2t_count_exact', (X, A, 4, 4, 4, A, A, 2, A, A, 1, 8, A, A, A, A, A, 0,), -2, 'laff_v2t_count_exact: list_cap must be >= 1'),
    ('laff_v2t_count_exact', (None, A, 4, 4, 4, A, A, 2, A, A, 1, 8, A, A, A, A, A, 16,), -1, 'laff_v2t_count_exact: null ctx'),
    ('laff_row_dot_gt', (X, None, None, 0, 4, 8, 1.0, 1, None, 0, None, None,), 0, ''),
    ('laff_row_dot_gt', (X, None, A, 4, 4, 8, 1.0, 1, A, 0, A, None,), -1, 'laff_row_dot_gt: null argument'),
    ('laff_row_dot_gt', (X, A, None, 4, 4, 8, 1.0, 1, A, 0, A, None,), -1, 'laff_row_dot_gt: null argument'),
    ('laff_row_dot_gt', (X, A, A, 4, 4, 8, 1.0, 1, None, 0, A, None,), -1, 'laff_row_dot_gt: null argument'),
    ('laff_row_dot_gt', (X, A, A, 4, 4, 8, 1.0, 1, A, 0, None, None,), -1, 'laff_row_dot_gt: null argument'),
    ('laff_row_dot_gt', (X, A, A, 4, 4, 8, 1.0, 0, A, 0, A, None,), -5, 'laff_row_dot_gt: 16-bit precisions only (got 0)'),
    ('laff_row_dot_gt', (X, A, A, 4, 4, 8, 1.0, 5, A, 0, A, None,), -5, 'laff_row_dot_gt: 16-bit precisions only (got 5)'),
    ('laff_row_dot_gt', (X, A, A, 4, 4, 8, 1.0, -1, A, 0, A, None,), -5, 'laff_row_dot_gt: 16-bit precisions only (got -1)'),
    ('laff_row_dot_gt', (X, A, A, -1, 4, 8, 1.0, 3, A, 0, A, A,), -2, 'laff_row_dot_gt: K must be positive and even (K=8)'),
    ('laff_row_dot_gt', (X, A, A, 4, -1, 8, 1.0, 3, A, 0, A, A,), -2, 'laff_row_dot_gt: K must be positive and even (K=8)'),
    ('laff_row_dot_gt', (X, A, A, 4, 4, 0, 1.0, 3, A, 0, A, A,), -2, 'laff_row_dot_gt: K must be positive and even (K=0)'),
    ('laff_row_dot_gt', (X, A, A, 4, 4, 7, 1.0, 3, A, 0, A, A,), -2, 'laff_row_dot_gt: K must be positive and even (K=7)'),
    ('laff_row_dot_gt', (X, A, A, 4, 4, 1, 1.0, 3, A, 0, A, A,), -2, 'laff_row_dot_gt: K must be positive and even (K=1)'),
    ('laff_row_dot_gt', (X, U, A, 4, 4, 8, 1.0, 1, A, 0, A, None,), -3, 'laff_row_dot_gt: operands must be 16-byte aligned'),
    ('laff_row_dot_gt', (X, A, U, 4, 4, 8, 1.0, 4, A, 0, A, None,), -3, 'laff_row_dot_gt: operands must be 16-byte aligned'),
    ('laff_row_dot_gt', (None, A, A, 4, 4, 8, 1.0, 1, A, 0, A, None,), -1, 'laff_row_dot_gt: null ctx'),
    ('laff_rank_metrics', (X, None, 4, 0, None, D8,), -1, 'laff_rank_metrics: null argument'),
    ('laff_rank_metrics', (X, A, 4, 0, None, None,), -1, 'laff_rank_metrics: null argument'),
    ('laff_rank_metrics', (X, A, 0, 1, None, D8,), -2, 'laff_rank_metrics: Nq=0'),
    ('laff_rank_metrics', (X, A, -2, 1, A, D8,), -2, 'laff_rank_metrics: Nq=-2'),
    ('laff_rank_metrics', (None, A, 4, 0, None, D8,), -1, 'laff_rank_metrics: null ctx'),
    ('laff_rank_metrics_async', (X, None, 4, 0, None, D8,), -1, 'laff_rank_metrics_async: null argument'),
    ('laff_rank_metrics_async', (X, A, 4, 0, None, None,), -1, 'laff_rank_metrics_async: null argument'),
    ('laff_rank_metrics_async', (X, A, 0, 1, None, D8,), -2, 'laff_rank_metrics_async: Nq=0'),
    ('laff_rank_metrics_async', (X, A, -2, 1, A, D8,), -2, 'laff_rank_metrics_async: Nq=-2'),
    ('laff_rank_metrics_async', (None, A, 4, 0, None, D8,), -1, 'laff_rank_metrics_async: null ctx'),
    ('laff_fuse_packed_rank', (X, None, 1, 4, 1, 8, A, A, None, 0, A, None, A, 1, 1.0, side(side=0),), -1, 'laff_fuse_packed_rank: side must be 1 (text) or 2 (video)'),
    ('laff_fuse_packed_rank', (X, None, 1, 4, 1, 8, A, A, None, 0, A, None, A, 1, 1.0, side(side=3),), -1, 'laff_fuse_packed_rank: side must be 1 (text) or 2 (video)'),
    ('laff_fuse_packed_rank', (X, None, 1, 4, 1, 8, A, A, None, 0, A, None, None, 1, 1.0, side(),), -5, 'laff_fuse_packed_rank: needs the 16-bit operand (E16) and split heads of d <= 512 (H=1 d=8): use laff_rank_prepare'),
    ('laff_fuse_packed_rank', (X, None, 1, 4, 1, 1024, A, A, None, 0, A, None, A, 1, 1.0, side(),), -5, 'laff_fuse_packed_rank: needs the 16-bit operand (E16) and split heads of d <= 512 (H=1 d=1024): use laff_rank_prepare'),
    ('laff_fuse_packed_rank', (X, None, 1, 4, 1, 8, A, A, None, 8, A, None, A, 1, 1.0, side(),), -5, 'laff_fuse_packed_rank: needs the 16-bit operand (E16) and split heads of d <= 512 (H=1 d=8): use laff_rank_prepare'),
    ('laff_fuse_packed_rank', (X, None, 1, 4, 1, 8, A, A, None, 0, A, None, None, 1, 1.0, side(side=2),), -5, 'laff_fuse_packed_rank: needs the 16-bit operand (E16) and split heads of d <= 512 (H=1 d=8): use laff_rank_prepare'),
    ('laff_fuse_packed_rank', (X, None, 1, 4, 2, 8, A, A, None, 0, A, None, A, 1, 1.0, side(partials=None),), -1, 'laff_fuse_packed_rank: several heads need the partials / tickets scratch'),
    ('laff_fuse_packed_rank', (X, None, 1, 4, 2, 8, A, A, None, 0, A, None, A, 1, 1.0, side(tickets=None),), -1, 'laff_fuse_packed_rank: several heads need the partials / tickets scratch'),
    ('laff_fuse_packed_rank', (X, None, 1, 4, 3, 8, A, A, None, 0, A, None, A, 1, 1.0, side(side=2, partials=None),), -1, 'laff_fuse_packed_rank: several heads need the partials / tickets scratch'),
    ('laff_fuse_packed_rank', (X, None, 1, 4, 1, 8, A, A, None, 0, A, None, A, 1, 1.0, side(band=None),), -1, 'laff_fuse_packed_rank: null band'),
    ('laff_fuse_packed_rank', (X, None, 1, 4, 1, 8, A, A, None, 0, A, None, A, 1, 1.0, side(side=2, band=None),), -1, 'laff_fuse_packed_rank: null band'),
    ('laff_fuse_packed_rank', (X, None, 1, 4, 1, 8, A, A, None, 0, A, None, A, 1, 1.0, side(gt_col=None),), -1, 'laff_fuse_packed_rank: the text side needs gt_col, Ev, s_gt64, band_v, count and pairs'),
    ('laff_fuse_packed_rank', (X, None, 1, 4, 1, 8, A, A, None, 0, A, None, A, 1, 1.0, side(Ev=None),), -1, 'laff_fuse_packed_rank: the text side needs gt_col, Ev, s_gt64, band_v, count and pairs'),
    ('laff_fuse_packed_rank', (X, None, 1, 4, 1, 8, A, A, None, 0, A, None, A, 1, 1.0, side(s_gt64=None),), -1, 'laff_fuse_packed_rank: the text side needs gt_col, Ev, s_gt64, band_v, count and pairs'),
    ('laff_fuse_packed_rank', (X, None, 1, 4, 1, 8, A, A, None, 0, A, None, A, 1, 1.0, side(band_v=None),), -1, 'laff_fuse_packed_rank: the text side needs gt_col, Ev, s_gt64, band_v, count and pairs'),
    ('laff_fuse_packed_rank', (X, None, 1, 4, 1, 8, A, A, None, 0, A, None, A, 1, 1.0, side(count=None),), -1, 'laff_fuse_packed_rank: the text side needs gt_col, Ev, s_gt64, band_v, count and pairs'),
    ('laff_fuse_packed_rank', (X, None, 1, 4, 1, 8, A, A, None, 0, A, None, A, 1, 1.0, side(pairs=None),), -1, 'laff_fuse_packed_rank: the text side needs gt_col, Ev, s_gt64, band_v, count and pairs'),
    ('laff_fuse_packed_rank', (X, None, 1, 4, 1, 8, A, A, None, 0, A, None, A, 1, 1.0, side(Nv=0),), -5, 'laff_fuse_packed_rank: 4 text rows cannot finish the block maxima of 0 videos: use laff_rank_prepare'),
    ('laff_fuse_packed_rank', (X, None, 1, 4, 1, 8, A, A, None, 0, A, None, A, 1, 1.0, side(Nv=-1),), -5, 'laff_fuse_packed_rank: 4 text rows cannot finish the block maxima of -1 videos: use laff_rank_prepare'),
    ('laff_fuse_packed_rank', (X, None, 1, 1, 1, 8, A, A, None, 0, A, None, A, 1, 1.0, side(Nv=17),), -5, 'laff_fuse_packed_rank: 1 text rows cannot finish the block maxima of 17 videos: use laff_rank_prepare'),
    ('laff_fuse_packed_rank', (X, None, 1, 4, 1, 8, A, A, None, 0, A, None, A, 1, 1.0, side(Ev=U),), -3, 'laff_fuse_packed_rank: Ev must be 16-byte aligned'),
    ('laff_fuse_packed_rank', (None, None, 1, 4, 1, 8, A, A, None, 0, A, None, A, 1, 1.0, side(),), -1, 'laff_fuse_packed_rank: null ctx'),
]


def test_the_table_reaches_every_entry_point_and_launches_nothing():
    want = {'laff_packed_bytes', 'laff_pack_rows', 'laff_sim_gemm', 'laff_sim_gemm_banded', 'laff_sim_gemm_route', 'laff_rank_prepare',
            'laff_rank_prepare_part', 'laff_rank_prepare_emit', 'laff_rank_export_pairs', 'laff_rank_resolve', 'laff_rank_resolve_metrics',
            'laff_gather_gt', 'laff_rank_count', 'laff_topk_rows', 'laff_v2t_count', 'laff_v2t_count_exact', 'laff_row_dot_gt',
            'laff_rank_metrics', 'laff_rank_metrics_async', 'laff_fuse_packed_rank'}
    assert {c[0] for c in CASES} == want
    for name, args, code, msg in CASES:
        assert code in (0, -1, -2, -3, -5) and (code == 0) == (msg == ''), (name, msg)
        if name != 'laff_packed_bytes':                                   # (the only one without a context)
            assert (args[0] is None) == msg.endswith(': null ctx'), (name, msg)
    for name in want - {'laff_packed_bytes'}:                             # the null context is checked last
        assert [c for c in CASES if c[0] == name][-1][3].endswith(': null ctx')


@pytest.mark.parametrize('name', sorted({c[0] for c in CASES}))
def test_refusals_and_empty_problems(name):
    lib = _lib.load()
    for entry, args, code, msg in CASES:
        if entry != name:
            continue
        got = getattr(lib, entry)(*args)
        assert (got, lib.laff_last_error().decode() if got else '') == (code, msg), (entry, args)


@pytest.mark.parametrize('Nv', [0, 1, 3, 4, 63, 64, 65, 1000])
@pytest.mark.parametrize('Nt', [0, 1, 3, 4, 63, 64, 65, 1000])
def test_rank_state_buffers_have_the_sizes_the_banded_gemm_reads(Nt, Nv):
    cpu = torch.device('cpu')
    s_gt64, band_t = ops._alloc_text_bands(Nt, cpu)
    assert s_gt64.dtype == torch.float64 and s_gt64.shape == (Nt,) and s_gt64.untyped_storage().nbytes() == 8 * (Nt + 2)
    assert band_t.dtype == torch.float32 and band_t.shape == (Nt + 4,)
    band_v = ops._alloc_band_v(Nv, cpu)
    assert band_v.dtype == torch.float32 and band_v.shape == (((Nv + 3) & ~3) + (Nv + 63) // 64 + 4,)
    for pair_cap, cap in ((None, max(1 << 20, 128 * Nt)), (4, 4), (7, 4), (8, 8), (1001, 1000)):
        if pair_cap is None and Nv:                                       # (the default list is 8 MiB: once per Nt)
            continue
        count, pairs, got = ops._alloc_list(Nt, pair_cap, cpu)
        assert got == cap and count.dtype == pairs.dtype == torch.int32 and count.shape == (Nt,) and pairs.shape == (4 + 2 * cap,)
    for pair_cap in (0, 3, -4):
        with pytest.raises(ValueError, match='pair_cap must be >= 4'):
            ops._alloc_list(Nt, pair_cap, cpu)


def test_optional_scores_and_pinned_result_arguments():
    assert ops._opt_scores(None) == (None, 0)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops._opt_scores(torch.zeros(2, 3))
    for bad in (torch.zeros(8, dtype=torch.float32), torch.zeros(7, dtype=torch.float64), torch.zeros(8, dtype=torch.float64)):
        with pytest.raises(ValueError, match='pinned float64 tensor of >= 8'):
            ops._pinned8(bad)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops._gt_col(torch.zeros(4, dtype=torch.int32))
