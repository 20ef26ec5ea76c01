"""`qg_twist_pack_words` refuses bad arguments before it touches the device: the checks of include/qgym.h on made-up addresses that are never
dereferenced, so this runs without a GPU (the same table runs on real buffers in test_gpu_twist_words.py)."""
from qiskit_gym_amd import _lib

W, P, T, O = 0x10000, 0x20000, 0x30000, 0x40000  # words, table, twist indices, output: aligned, never read


def test_pack_words_argument_checks_need_no_device():
    call = _lib.load().qg_twist_pack_words
    invalid = [(None, 8, 4, 8, 8, P, 2, T, O, 8), (W, 8, 4, 8, 8, None, 2, T, O, 8), (W, 8, 4, 8, 8, P, 2, None, O, 8), (W, 8, 4, 8, 8, P, 2, T, None, 8),
               (W, 8, 0, 8, 8, P, 2, T, O, 8), (W, 8, 4, 0, 8, P, 2, T, O, 8), (W, 8, 4, 8, 0, P, 2, T, O, 8), (W, 8, 4, 8, 8, P, 0, T, O, 8),
               (W, 8, 4, 8, 8, P, 2, T, O, 0),
               (W, 2, 4, 8, 8, P, 2, T, O, 8), (W, 16, 4, 8, 8, P, 2, T, O, 8),   # word_bytes
               (W, 8, 4, 8, 65, P, 2, T, O, 8), (W, 4, 4, 8, 33, P, 2, T, O, 8), (W, 1, 4, 8, 257, P, 2, T, O, 8),  # cols that do not fit the word
               (W, 8, 4, 8, 8, P, 2, T, O + 4, 8), (W + 4, 8, 4, 8, 8, P, 2, T, O, 8), (W, 8, 4, 8, 8, P + 2, 2, T, O, 8), (W, 8, 4, 8, 8, P, 2, T + 1, O, 8)]
    for args in invalid:
        assert call(*args, None) == -1, args  # QG_ERR_INVALID
    unsupported = [(W, 1, 4, 8, 65, P, 2, T, O, 8),      # a byte names up to 256 columns, a word of the view holds 64
                   (W, 8, 4, 8, 8, P, 2, T, O, 7),       # rows_out < rows
                   (W, 8, 4, 8, 8, P, 2, T, O, 19),      # rows_out > 2 * rows + 2
                   (W, 8, 4, 257, 1, P, 2, T, O, 257),   # more than 2 KiB of words per env
                   (W, 4, 2**31, 8, 8, P, 2, T, O, 8),   # batch
                   (W, 1, 4, 2048, 64, P, 16384, T, O, 2048)]  # a table of 2^31 entries
    for args in unsupported:
        assert call(*args, None) == -3, args  # QG_ERR_UNSUPPORTED
    assert b"twist_pack_words" in _lib.load().qg_last_error()
