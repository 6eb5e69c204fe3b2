"""The records of front_cases.py on the CPU: the plain-Python rule (front_model.py) against the literals of the hand-built
cases, the oracle's front end against the rule on every record, and the ledger of shapes the generator must have produced.
test_gpu_front_edges.py runs the product over the same records."""
import difflib
import functools

import pytest

import front_cases as fc
import front_model as fm
from nextpolish2_amd import io as np2io
from nextpolish2_amd.bamio import read_bam, records_to_arrays, write_bam
from oracle import np2_oracle as orc


@functools.lru_cache(None)
def oracle_pileup(tid):
    """the oracle's pileup of contig tid's records (shared, never written to)"""
    recs, _, _ = fc.records(tid)
    arr, cig, seq4, asc, asc_off = records_to_arrays(recs)
    pu = orc.front_end(fc.contig(tid).encode(), arr, cig, asc, asc_off, fc.front_opts())
    for a in (pu.reads, pu.nibbles):
        a.setflags(write=False)
    return pu


def kept_names(tid):
    recs, model, _ = fc.records(tid)
    return [r["name"].decode() for r in recs if model[r["name"].decode()] is not None]


def pileup_against_model(pu, tid):
    """-> the names of the records whose entry in pileup `pu` is not what the rule gives (aln_t_s, aln_t_e, n_cols and the
    stream up to and including the terminator byte); entry 0 is the contig itself"""
    _, model, _ = fc.records(tid)
    names = kept_names(tid)
    want = [model[nm][2:] + (0,) for nm in names]
    got = []
    for rd in pu.reads[1:]:
        off, n_cols = int(rd["nib_off"]), int(rd["n_cols"])
        got.append((int(rd["aln_t_s"]), int(rd["aln_t_e"]), n_cols, pu.nibbles[off:off + n_cols // 2 + 1].tobytes(), int(rd["flags"])))
    if got == want:
        return []
    # entries are in the records' order; where one is missing or one too many, line the two lists up again behind it
    bad = []
    for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, want, got, autojunk=False).get_opcodes():
        if tag != "equal":
            bad += names[i1:i2] if i2 > i1 else ["(%d entries no record gives, before %s)" % (j2 - j1, (names + ["the end"])[i1])]
    return bad


@pytest.mark.parametrize("tid", [0, 1])
def test_model_gives_the_literals_of_the_named_cases(tid):
    _, model, _ = fc.records(tid)
    seen = 0
    for name, (_, _, exp, only) in fc.NAMED.items():
        if only is not None and only != tid:
            continue
        seen += 1
        m = model[name]
        assert (None if m is None else m[:5]) == exp, name
        if m is not None:
            assert len(m[5]) == exp[4] // 2 + 1, name
            assert m[5][-1] == 0xFF if exp[4] % 2 == 0 else m[5][-1] & 0x0F == 0x0F, name
    assert seen == len(fc.NAMED) - 1
    at, nib = fc.ALL_CODES_NIBBLES
    assert model["all_codes"][5].hex()[at:at + len(nib)] == nib


@pytest.mark.parametrize("tid", [0, 1])
def test_oracle_front_end_equals_the_model(tid):
    recs, model, _ = fc.records(tid)
    assert [r["pos"] for r in recs] == sorted({r["pos"] for r in recs})  # every record its own POS, ascending
    assert pileup_against_model(oracle_pileup(tid), tid) == []


@pytest.mark.parametrize("tid", [0, 1])
def test_generator_ledger(tid):
    """every shape the named cases pin is met in the generated records too"""
    recs, model, g = fc.records(tid)
    assert g["first_lane"] >= {0, 1} and g["first_chunk"] >= {0, 1} and g["last_chunk"] >= {0, 1, 2}
    assert g["last_chunk_from_end"] >= {0, 1}  # a backward search that ends in the last pass, and one that ends before it
    for k in ("first_over_lane", "first_over_chunk", "last_over_lane", "last_over_chunk", "n_cols_mod2048_is_0"):
        assert g[k] == {False, True}, k
    assert g["n_cols_mod32"] >= {0, 15, 16, 31}
    assert g["n_cols"] >= {8, 9, 15, 16, 17, 31, 32, 33, 2047, 2048, 2049, 4096}
    assert g["shift_parity_at"] >= {(16, 0), (16, 1), (2048, 0), (2048, 1)}
    # a condition, not a measurement: no generated record loses its anchor by accident
    assert g["without_anchor"] == g["built_without_anchor"] > 0
    assert g["kept"] + g["without_anchor"] == 400
    named_without = sum(1 for nm, (_, _, exp, only) in fc.NAMED.items() if exp is None and only in (None, tid))
    assert sum(1 for m in model.values() if m is None) == g["built_without_anchor"] + named_without


@pytest.mark.parametrize("op", ["N", "P"])
def test_n_and_p_ops_panic(op):
    rec = fc.panic_record(0, op)
    with pytest.raises(fm.UnknownCigar):
        fm.columns(fc.contig(0), rec)
    arr, cig, seq4, asc, asc_off = records_to_arrays([rec])
    with pytest.raises(orc.RefPanic):
        orc.front_end(fc.contig(0).encode(), arr, cig, asc, asc_off, fc.front_opts())


def test_bam_cut_at_a_byte_limit_reads_back(tmp_path):
    """block_limit=300: every record, its length word and its fixed fields are split between blocks"""
    recs = fc.records(0)[0][:60] + fc.records(1)[0][:60]
    path = str(tmp_path / "cut.bam")
    write_bam(path, fc.REFS, recs, block_limit=300, level=6)
    refs, back = read_bam(path)
    assert refs == fc.REFS and len(back) == len(recs)
    for a, b in zip(back, recs):
        want = dict(b, seq="".join(fm.bam_letter(c) for c in b["seq"]))
        assert a == want, b["name"]
    assert np2io.Bam(path).refs() == fc.REFS
    # the default is what it was: blocks end on record boundaries
    write_bam(str(tmp_path / "whole.bam"), fc.REFS, recs)
    assert read_bam(str(tmp_path / "whole.bam"))[1] == back
