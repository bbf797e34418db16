"""The kernels of the DEFLATE encoder (k_tgz_match / k_tgz_codes / k_tgz_bits, svim_amd/csrc/textgz_kernels.hpp) held to the encoder's definition in plain Python
(tests/deflate_model.py) on the directed cases of tests/deflate_encode_cases.py: one call of svx_text_gz_phase per phase over all cases of that phase (one wave per
block), and svx_text_gz with the texts as the files of one call.  The host build's twin of every check: tests/test_deflate_encode_cases.py."""
import numpy as np
import pytest

import deflate_encode_cases as DC
import deflate_model as M
from test_deflate_encode_cases import check_bits, check_codes, check_match

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from svim_amd import _lib
    return _lib.engine()


def test_match_kernel_equals_the_model(eng):
    from svim_amd import _lib
    mb = DC.match_batch()
    check_match(_lib.text_gz_phase("match", mb["n"], mb["text"], mb["off"], engine=eng), mb)


def test_codes_kernel_equals_the_model(eng):
    from svim_amd import _lib
    cb = DC.codes_batch()
    check_codes(_lib.text_gz_phase("codes", cb["n"], hist=cb["hist"], crc=cb["crc"], engine=eng), cb)


def test_bits_kernel_equals_the_model(eng):
    from svim_amd import _lib
    bb = DC.bits_batch()
    check_bits(_lib.text_gz_phase("bits", bb["n"], bb["text"], bb["off"], tok=DC.strided_tokens(bb["tok"]), nt=bb["nt"], codes=bb["codes"], engine=eng), bb)


def test_text_gz_of_all_texts_equals_the_model_twice_and_inflates_on_the_device(eng, tmp_path):
    """the texts as the files of one svx_text_gz call (their starts at all four alignments): every file's stream = the model's block + the end-of-file block; the
    same call again gives the same bytes; svx_inflater_run reads the stream back to the texts"""
    from svim_amd import _abi, _lib
    mb = DC.match_batch()
    texts, names, size = [], [], 0
    for k, (name, t) in enumerate(zip(mb["names"], mb["texts"])):
        if size % 4 != k % 4:                                          # a file of one to three bytes in front: the k-th text starts at k mod 4
            texts.append(b"Z" * ((k - size) % 4)), names.append("pad in front of " + name)
            size += len(texts[-1])
        assert size % 4 == k % 4
        texts.append(t), names.append(name)
        size += len(t)
    data = b"".join(texts)
    off = np.cumsum([0] + [len(t) for t in texts])
    want = {}
    for t in set(texts):
        want[t] = DC.model_block(t) + M.EOF_BLOCK
    streams = []
    for _ in range(2):
        assert eng.text_gz(_abi.TEXT_GZ_HOST, data, off)[0] == len(texts)
        streams.append(eng.text_gz_fetch())
    fo = eng.text_gz_tables()[0]
    for k, (name, t) in enumerate(zip(names, texts)):
        assert streams[0][int(fo[k]):int(fo[k + 1])] == want[t], name
    assert streams[0] == streams[1]
    path = str(tmp_path / "all.gz")
    with open(path, "wb") as fh:
        fh.write(streams[0])
    f = _lib.Inflater(0)
    try:
        assert f.inflate(_lib.bgzf_blocks(path)).tobytes() == data
    finally:
        f.close()
