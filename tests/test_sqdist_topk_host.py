"""SSCDR's distance score under the fused mask + top-k (cdr_fullsort_neg_sqdist_topk_f32), the parts that need no GPU: the workspace is
the dot-product entry's -- one plan serves both scores -- plus the two norm vectors; a refused query writes nothing and names itself;
SSCDR, CLFM and DCDCSR evaluate through ``full_sort_topk`` like the other seven models.  Only the query entries are called: nothing here
can launch."""
import ctypes

import pytest

from recbole_cdr_amd import binding, get_model

US = (1, 8, 33, 64, 513)
DS = (32, 64, 128)
SLABS = ((64, 0), (9000, 0), (13333, 26667), (0, 70001))
KS = (1, 10, 64)
NAME = 'cdr_fullsort_neg_sqdist_topk_workspace_bytes'


def test_workspace_is_the_dot_product_workspace_plus_the_norm_vectors():
    lib = binding.load()
    dot, sq, bad = ctypes.c_size_t(0), ctypes.c_size_t(0), []
    for U in US:
        for D in DS:
            for n0, n1 in SLABS:
                for k in KS:
                    assert lib.cdr_fullsort_topk_workspace_bytes(U, D, n0, n1, k, ctypes.byref(dot)) == 0, lib.cdr_last_error()
                    assert getattr(lib, NAME)(U, D, n0, n1, k, ctypes.byref(sq)) == 0, lib.cdr_last_error()
                    want = dot.value + ((4 * (U + n0 + n1) + 255) & ~255)
                    if sq.value != want:
                        bad.append((U, D, n0, n1, k, sq.value, want))
    assert not bad, f'{len(bad)} sizes differ; first (U, D, n0, n1, k, got, want): {bad[:5]}'


@pytest.mark.parametrize('U,n0,n1,k', [(64, 1000, 0, 0), (64, 1000, 0, 65), (0, 1000, 0, 10), (64, 0, 0, 10)])
def test_workspace_query_refusals_write_nothing_and_name_the_function(U, n0, n1, k):
    lib, need = binding.load(), ctypes.c_size_t(12345)
    assert getattr(lib, NAME)(U, 64, n0, n1, k, ctypes.byref(need)) != 0
    assert NAME.encode() in lib.cdr_last_error()
    assert need.value == 12345


def test_workspace_query_refuses_a_null_result_pointer():
    lib, need = binding.load(), ctypes.c_size_t(12345)
    assert getattr(lib, NAME)(64, 64, 1000, 0, 10, None) != 0
    assert NAME.encode() in lib.cdr_last_error()
    assert getattr(lib, NAME)(64, 64, 1000, 0, 10, ctypes.byref(need)) == 0 and need.value not in (0, 12345)


def test_the_entry_refuses_before_it_launches():
    """Out-of-range arguments, a short workspace and the few-users shapes the entry has no form for (U <= 8 where the dot-product entry
    streams a GEMV: ``F_.fullsort_neg_sqdist_topk`` pads those to nine rows) are refused with a text that names the entry.  The pointers are
    host memory that nothing reads: a refusal comes before the first launch, so this runs without a GPU."""
    lib = binding.load()
    fn, name = lib.cdr_fullsort_neg_sqdist_topk_f32, b'cdr_fullsort_neg_sqdist_topk_f32'
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    big = 1 << 40

    def call(U=64, D=64, n0=1000, n1=0, k=10, ws=big, indptr=None, cols=None, slab0=p):
        return fn(None, p, U, D, slab0, n0, None, n1, None, k, indptr, cols, 1, p, p, p, ws)
    for kw in (dict(k=0), dict(k=65), dict(U=0), dict(slab0=None), dict(n0=5, k=10), dict(n0=1 << 31), dict(indptr=p), dict(ws=1024),
               dict(U=5), dict(U=8, D=128, n0=70001)):
        assert call(**kw) == -1, kw                                  # CDR_EINVAL (a failed launch would hand back HIP's positive code)
        assert name in lib.cdr_last_error(), (kw, lib.cdr_last_error())


@pytest.mark.parametrize('name', ['SSCDR', 'CLFM', 'DCDCSR'])
def test_the_three_models_evaluate_through_full_sort_topk(name):
    cls = get_model(name)
    assert callable(getattr(cls, 'full_sort_topk')) and callable(getattr(cls, 'full_sort_predict'))


@pytest.mark.parametrize('name', ['CMF', 'CLFM', 'BiTGCF', 'DCDCSR'])
def test_a_contraction_model_states_its_operands_and_inherits_the_routes(name):
    """These four score the plain dot of ``_full_sort_operands``: the routes come from ``ContractionScoring``, not from copies per model."""
    from recbole_cdr_amd.model.contraction import ContractionScoring
    cls = get_model(name)
    assert '_full_sort_operands' in vars(cls)
    assert 'full_sort_predict' not in vars(cls) and 'full_sort_topk' not in vars(cls)
    assert cls.full_sort_predict is ContractionScoring.full_sort_predict and cls.full_sort_topk is ContractionScoring.full_sort_topk


def test_sscdr_brackets_an_evaluation():
    cls = get_model('SSCDR')
    assert callable(getattr(cls, 'freeze_for_eval')) and callable(getattr(cls, 'unfreeze_eval'))
    assert callable(getattr(cls, '_full_sort_operands'))
