"""memo_amd._window.parse_region without a GPU: every driver reads `-r CHR:START-END` through it, and what is wrong with a region
raises what `memo query` raises for it -- the exceptions below are what collect.parse_region raised before the parser had one home."""
import pytest

MALFORMED = [
    ("chr1", "not enough values to unpack (expected 2, got 1)"),                 # no ':'
    ("chr1:5", "not enough values to unpack (expected 2, got 1)"),               # no '-'
    ("a:b:1-2", "too many values to unpack (expected 2)"),                       # two ':'
    ("chr1:1-2-3", "too many values to unpack (expected 2)"),                    # two '-'
    ("chr1:-5-3", "invalid literal for int() with base 10: ''"),                 # a sign is a second '-': int() sees the empty start first
    ("chr1:x-3", "invalid literal for int() with base 10: 'x'"),
    ("chr1:9-3", "negative dimensions are not allowed"),                         # a reversed window
]


@pytest.mark.parametrize("region, message", MALFORMED)
def test_a_malformed_region_raises_what_memo_query_raises(region, message):
    from memo_amd._window import parse_region
    with pytest.raises(ValueError) as caught:
        parse_region(region)
    assert type(caught.value) is ValueError and str(caught.value) == message


def test_a_region_is_record_start_end():
    from memo_amd._window import parse_region
    assert parse_region("chr1:3-3") == ("chr1", 3, 3)                            # an empty window is a window
    assert parse_region("chr1:0-7") == ("chr1", 0, 7)


def test_collect_keeps_its_name_for_the_parser():
    from memo_amd import _window, collect
    assert collect.parse_region is _window.parse_region
