"""CPU tests of the long-code configurations (tests/synth_stream.py: LONGCODE_NAMES): that each book reaches the parser route
it exists for, and that the structured streams write every code of every book.

Both parsers decode a symbol along a route chosen per book at stream open (host_setup.cpp: generate_table; nvh_setup.hip:
plan_parse_tables).  The routes are read back through nvh_stream_parse_book_info, on a host-only stream, instead of being
recomputed here from the thresholds: a constant that moves then fails these assertions rather than silently leaving a branch
unvisited.  The decodes themselves are compared in test_host_logic.py (tables), test_host_slabs.py (host parser == oracle, bit
for bit), test_spec_pin.py (oracle == specification) and, on the GPU, test_gpu_parse.py.
"""
import ctypes as C

import pytest

from tests import spec_pin, synth_stream as ss, vorbis_encode as ve

LDS, NODES, SUB, ALL, HOST = "prefix_in_lds", "overflow_in_lds", "second_level", "scan_all_slots", "host_scan_slots"

# configuration -> book -> what the query must report (keys left out are not part of the book's purpose)
ROUTES = {
    "longcode_res1": {
        11: {LDS: 1, NODES: 1, SUB: 1, ALL: 0, HOST: 0},   # classbook: the class-word path's second-level lookup
        12: {LDS: 1, NODES: 1, SUB: 1, ALL: 0, HOST: 0},   # floor1 masterbook
        13: {LDS: 1, NODES: 1, SUB: 1, ALL: 0, HOST: 0},   # floor1 subclass book, ordered
        14: {LDS: 1, NODES: 1, SUB: 0, ALL: 0, HOST: 0},   # ladder: a group 21 bits deep -> its group scanned in LDS
        15: {LDS: 1, NODES: 1, SUB: 1, ALL: 0, HOST: 0},   # 512 small groups -> second-level tables
        16: {LDS: 1, NODES: 1, SUB: 1, ALL: 0, HOST: 0},   # lattice with long codes
        17: {LDS: 1, SUB: 0, ALL: 1, HOST: 0},             # a group of 200: GPU scans the whole list, the host the group
        18: {LDS: 1, SUB: 0, ALL: 1, HOST: 1},             # a group of 256: both scan the whole list
        19: {LDS: 1, NODES: 1, SUB: 1, ALL: 0, HOST: 0},   # sparse, stays sparse
        20: {LDS: 1, NODES: 1, SUB: 1, ALL: 0, HOST: 0},   # sparse, converted
        21: {LDS: 1, NODES: 1, SUB: 0, ALL: 0, HOST: 0},   # ladder, ordered: max_bits 32
    },
    "longcode_res2": {
        11: {LDS: 1, NODES: 1, SUB: 1, ALL: 0, HOST: 0},
        12: {LDS: 1, NODES: 1, SUB: 1, ALL: 0, HOST: 0},
        13: {LDS: 1, NODES: 1, SUB: 1, ALL: 0, HOST: 0},
        14: {LDS: 1, NODES: 0, SUB: 0, ALL: 0, HOST: 0},   # 4096 nodes: groups scanned in global memory
        15: {LDS: 1, NODES: 1, SUB: 0, ALL: 0, HOST: 0},   # a group 14 bits deep
        16: {LDS: 1, NODES: 1, SUB: 0, ALL: 0, HOST: 0},   # two groups 12 bits deep: the second-level image is full
        17: {LDS: 1, NODES: 1, SUB: 1, ALL: 0, HOST: 0},   # lattice 3^4
        18: {LDS: 1, NODES: 1, SUB: 1, ALL: 0, HOST: 0},   # dimension 3, explicit table
        19: {LDS: 1, NODES: 1, SUB: 1, ALL: 0, HOST: 0},   # lattice 3^3
        20: {LDS: 1, NODES: 1, SUB: 1, ALL: 0, HOST: 0},   # explicit table, sparse
    },
}


def _stream(name):
    import nvorbis_amd as nv
    hdr = spec_pin.headers(name)
    return nv.Stream(None, hdr[0], hdr[1], hdr[2])


def _book_info(st, b):
    import nvorbis_amd as nv
    v = [C.c_int(0) for _ in range(7)]
    assert nv.lib().nvh_stream_codebook_info(st._h, b, *[C.byref(x) for x in v]) == 0
    return dict(zip(("dims", "entries", "map_type", "prefix_bits", "max_bits", "n_prefix", "n_overflow"), (x.value for x in v)))


@pytest.mark.parametrize("name", sorted(ROUTES))
def test_every_book_takes_the_route_it_exists_for(name):
    st = _stream(name)
    try:
        for b, want in ROUTES[name].items():
            got = st.parse_book_info(b)
            assert got["gpu_parse_ok"] == 1, name
            assert {k: got[k] for k in want} == want, (name, b, got)
            assert _book_info(st, b)["n_overflow"] > 0, (name, b)  # every one of them has codes past the prefix table
        # the books of the older configurations, eight bits at the most: no overflow list, nothing to route
        for b in range(11):
            got = st.parse_book_info(b)
            assert (got[NODES], got[SUB], got[ALL], got[HOST]) == (0, 0, 0, 0) and _book_info(st, b)["n_overflow"] == -1
    finally:
        st.close()


def test_ladder_lengths_and_the_ordered_off_by_one():
    """The dense ladder reports max_bits 31, the ordered one the reference's 32 (Codebook.cs:84-99 leaves `len` one past the last
    run): the value at which the parser masks the peeked word."""
    st = _stream("longcode_res1")
    try:
        assert _book_info(st, 14)["max_bits"] == 31 and _book_info(st, 21)["max_bits"] == 32
        assert _book_info(st, 13)["max_bits"] == 13  # the ordered floor book, lengths 1, 11, 12, 12
        assert _book_info(st, 19)["entries"] == 64 and _book_info(st, 20)["entries"] == 64
    finally:
        st.close()


def test_books_left_out_of_lds():
    """Eighteen residue books with a 1024-slot prefix table each: some keep theirs in global memory, and both residues use books of
    either kind, so that a frame's walk mixes fast and NVH_PVIS_SLOW visits."""
    st = _stream("longcode_many_books")
    try:
        info = {b: st.parse_book_info(b) for b in range(11, 29)}
        assert all(i["gpu_parse_ok"] == 1 for i in info.values())
        out = {b for b, i in info.items() if not i[LDS]}
        assert out and len(out) < 18, out
        for b in out:  # a book without its prefix table in LDS has nothing else there
            assert info[b][NODES] == 0 and info[b][SUB] == 0
        S = ve.setup_of(list(spec_pin.headers("longcode_many_books")))
        for res in S.residues:
            used = {bk for row in res.books for bk in row if bk >= 0}
            assert used & out and used - out, (used, out)
    finally:
        st.close()


def test_query_checks_its_arguments():
    import nvorbis_amd as nv
    from nvorbis_amd import native
    st = _stream("longcode_res1")
    try:
        L = nv.lib()
        assert L.nvh_stream_parse_book_info(None, 0, None, None, None, None, None, None) == native.ERR_ARGUMENT
        for bad in (-1, 22):
            assert L.nvh_stream_parse_book_info(st._h, bad, None, None, None, None, None, None) == native.ERR_ARGUMENT
        assert L.nvh_stream_parse_book_info(st._h, 0, None, None, None, None, None, None) == 0
    finally:
        st.close()
    # a Floor0 setup is outside the GPU parser's limits: the query says so, and reports no GPU route
    hdr = spec_pin.headers("floor0_stereo")
    st = nv.Stream(None, hdr[0], hdr[1], hdr[2])
    try:
        got = st.parse_book_info(3)
        assert (got["gpu_parse_ok"], got[LDS], got[NODES], got[SUB], got[ALL]) == (0, 0, 0, 0, 0)
    finally:
        st.close()


@pytest.mark.parametrize("name", ss.LONGCODE_NAMES)
def test_structured_streams_write_every_code_length(name):
    """The encoder draws entries uniformly, so the long codes are written (random-bit packets essentially never contain a 20-bit
    code): every code length of every new book appears in the 24-frame stream, the classbook's and the floor books' included."""
    pk, _, stats = spec_pin.stream24(name)
    S = ve.setup_of(list(pk[:3]))
    sym = stats["symbols"]
    for b in range(11, len(S.books)):
        lens = sorted({w[1] for w in S.books[b].words if w is not None})
        assert max(lens) > 10, (name, b)
        missing = [n for n in lens if sym.get((b, n), 0) == 0]
        assert not missing, (name, b, missing)
    cut, _ = spec_pin.stream24_cut(name)
    shorter = [i for i in range(3, len(pk)) if len(cut[i]) < len(pk[i])]
    assert shorter == list(range(3, len(pk), 2))
    assert all(len(pk[i]) // 2 <= len(cut[i]) and cut[i] == pk[i][:len(cut[i])] for i in shorter)
