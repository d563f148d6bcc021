"""tests/kmeans_oracle.py, the plain-integer restatement of QuantizedKmeans,
on cases worked by hand: before anything is compared with it."""
import kmeans_oracle as o

U = o.U


def test_the_integer_cube_root_is_exact():
    for v, w in ((0, 0), (1, 1), (7, 1), (8, 2), (26, 2), (27, 3), (1 << 60, 1 << 20), (((1 << 20) + 1) ** 3 - 1, 1 << 20),
                 (((1 << 20) + 1) ** 3, (1 << 20) + 1), ((1 << 62) - 1, 1664510)):
        assert o.icbrt(v) == w, v
    assert 1664510 ** 3 <= (1 << 62) - 1 < 1664511 ** 3  # the largest argument: a bin that holds 2^32 elements


def test_the_image_spans_the_32_bits_and_rounds_half_to_even():
    assert o.image([0.0, 1.0], 0.0, 1.0) == [0, U]
    # 0.5 * (2^32 - 1) = 2147483647.5, exactly representable: the tie goes to the even 2147483648
    assert o.image([0.5], 0.0, 1.0) == [2147483648]
    # s = 1 for integer data over the whole range
    assert o.image([0.0, 7.0, 4294967294.0, float(U)], 0.0, float(U)) == [0, 7, U - 1, U]
    assert o.image([-3.0, 9.0], 0.0, 1.0) == [0, U]  # a start outside the range is clipped


def test_the_start_on_two_equal_bins():
    """h = 8 in the first and the last bin: w = icbrt(2^33) = 2048 each, tot = 4096.  K = 2: r = 1024 lies half
    way into bin 0, r = 3072 half way into bin 4095."""
    h = [0] * o.BINS
    h[0] = h[4095] = 8
    assert o.start(h, 2) == [1 << 19, (4095 << 20) + (1 << 19)]
    # K = 4: r = 512, 1536, 2560, 3584: a quarter and three quarters into either bin
    assert o.start(h, 4) == [1 << 18, 3 << 18, (4095 << 20) + (1 << 18), (4095 << 20) + (3 << 18)]


def test_the_start_weighs_bins_by_the_cube_root_of_their_count():
    """h = 1 and 27: w = 1024 and 3072 (cube roots of 2^30 and 27 * 2^30), tot = 4096.  K = 2: r = 1024 is the
    first value past bin 0 (W[0] = 1024 is not above it), so c_0 sits at the start of bin 1; r = 3072 lies
    2048 / 3072 = two thirds into bin 1."""
    h = [0] * o.BINS
    h[0], h[1] = 1, 27
    assert o.start(h, 2) == [1 << 20, (1 << 20) + (2048 << 20) // 3072]


def test_a_step_by_hand():
    # b_0 = (5 + 60) >> 1 = 32: 32 is ON the boundary and stays below, 33 goes up
    assert o.labels([0, 32, 33, 100], [5, 60]) == [0, 0, 1, 1]
    assert o.step([0, 10, 20, 100], [5, 60]) == [10, 100]
    # sum 1 over count 2: remainder exactly cnt / 2 rounds up; 7 over 3 (remainder 1 of 3) rounds down
    assert o.step([0, 1, 100], [0, 100]) == [1, 100]
    assert o.step([2, 2, 3, 100], [0, 100]) == [2, 100]
    # 8 over 3 (remainder 2 of 3) rounds up
    assert o.step([2, 3, 3, 100], [0, 100]) == [3, 100]
    # an empty cluster keeps its centre: b = (5 + 50) >> 1 = 27 and (50 + 100) >> 1 = 75
    assert o.step([0, 10, 90, 100], [5, 50, 100]) == [5, 50, 95]


def test_the_wrong_variants_are_wrong_where_they_should_be():
    assert o.labels([32], [5, 60], "le") == [1]
    assert o.step([0, 1, 100], [0, 100], "half_down") == [0, 100]
    assert o.step([0, U, U, U], [0, U], "sum32") == [0, (3 * U & 0xFFFFFFFF) // 3]


def test_a_fit_by_hand():
    """Two clumps of three: from the ends of the range the first step moves both centres to the clumps' means,
    the second moves nothing: n_iter = 2."""
    xs = [0.0, 1.0, 2.0, 10.0, 11.0, 12.0]
    labels, c, n_iter, q = o.fit(xs, 2, init=[0.0, 12.0])
    assert labels == [0, 0, 0, 1, 1, 1] and n_iter == 2
    us = o.image(xs, 0.0, 12.0)
    assert c == [us[1], us[4]]  # the middle elements: the others lie symmetric around them, up to a unit
    assert abs(q[0] - 1.0) < 1e-8 and abs(q[1] - 11.0) < 1e-8
    assert o.fit(xs, 2, init=[0.0, 12.0], max_iter=1)[2] == 1
