/* tbnav_icp.h — ICP between two laser scans on the GPU (point-to-point, and point-to-line as an option; a correlative search
 * for the initial guess as another): the scan matcher that the reference's
 * bmapping::ScanAlignment::pclICPWrapper (bmapping/src/bmapping/cloud_alignment.cpp:37-223) runs once per scan through
 * pcl::IterativeClosestPoint<PointXYZ, PointXYZ>.  PCL is a third-party library that is not part of this project, so
 * what is implemented here is a RESTATEMENT of PCL 1.8's algorithm with the reference's settings (max_iter 100,
 * max_correspondence_dist 0.5, transformation_epsilon 1e-8, euclidean_fitness_epsilon 1e-6; cloud_alignment.cpp:21-34,
 * 186-190).  Its arithmetic is fixed below tightly enough that a numpy restatement (tests/icp_restatement.py) reproduces
 * the kernel bit for bit.  Parity with PCL itself is UNPINNED: no PCL build has been compared against it.
 *
 * CONTRACT
 *  1. Cloud (createPointCloud, cloud_alignment.cpp:76-157).  float beam_angle starts at beam_min; beam i is kept when
 *     r >= range_min && r < range_max (float compares: NaN and inf fall out); its point is (double)r * (double)cosf(angle),
 *     (double)r * (double)sinf(angle), mapped by Trs as rigid2d::Transform2D::operator() does ((c*x - s*y) + tx,
 *     (s*x + c*y) + ty in fp64, c = cos(Trs theta), s = sin(Trs theta)) and rounded to float; then beam_angle +=
 *     beam_delta (float) and the wrap of :140-154 (beam_max < 0: angle <= beam_max -> beam_min; else angle >= beam_max ->
 *     beam_min).  The cosf/sinf table is built on the host with glibc once per beam count; the points on the device.
 *  2. Initial guess (pclICP, :171-183): R = [[c, -s], [s, c]], t = (x, y) with c = float(cos theta), s = float(sin theta),
 *     x = float(x), y = float(y) of T_init, held in fp64 from then on.
 *  3. Iteration k = 1, 2, ...:
 *     - every source point a0 goes to a = float(((R00*a0x) + (R01*a0y)) + tx), likewise y with R10, R11, ty (fp64, no
 *       contraction);
 *     - its nearest target point b: the fp32 d = dx*dx + dy*dy, targets scanned in beam order with a strict '<' (the lowest
 *       index wins a tie); the pair is kept when (double)d <= max_corr_dist * max_corr_dist (PCL drops d > max^2);
 *     - fewer than 3 pairs: FAILED (TBNAV_ICP_NO_CORRESPONDENCES);
 *     - fp64 sums n, Sax, Say, Sbx, Sby, Sax*bx, Say*by, Sax*by, Say*bx, Sd in this FIXED order: thread t of B = 256 adds the
 *       kept pairs of the source beams i = t, t + B, t + 2B, ... in increasing i (i is the BEAM index, invalid beams add
 *       nothing), then a tree adds t and t + s for s = B/2, ..., 1;
 *     - A = (Sax*bx + Say*by) - ((Sax*Sbx) + (Say*Sby)) / n,  S = (Sax*by - Say*bx) - ((Sax*Sby) - (Say*Sbx)) / n,
 *       r = sqrt((A*A) + (S*S)); r == 0: FAILED (TBNAV_ICP_DEGENERATE); else c = A/r, s = S/r,
 *       t_inc = b_mean - R_inc * a_mean (means = sums / n);
 *     - R <- R_inc * R, t <- R_inc * t + t_inc.  No transcendental inside the loop: in exact arithmetic this is the 2-D
 *       solution PCL's Umeyama SVD finds for points of constant z.
 *  4. Stopping, checked after the update in PCL's DefaultConvergenceCriteria order:
 *     k >= max_iter -> TBNAV_ICP_ITERATIONS (PCL counts this as converged);
 *     c >= 1 - transform_eps && |t_inc|^2 <= transform_eps -> TBNAV_ICP_TRANSFORM;
 *     mse = Sd / n of this iteration: |mse - prev| < 1e-12 -> TBNAV_ICP_ABS_MSE; |mse - prev| / prev < fitness_eps ->
 *     TBNAV_ICP_REL_MSE; otherwise prev = mse (prev starts at DBL_MAX).
 *  5. Result (host): theta = atan2(R10, R00), x = t0, y = t1.  On a failure T_out is (0, 0, 0).
 *
 * KNOWN DIVERGENCES FROM PCL
 *  - PCL applies each increment to the float cloud in place and evaluates its criteria in float; here the source points
 *    are transformed from the original cloud by the accumulated fp64 transform.
 *  - PCL's kd-tree breaks distance ties in its own order.
 *  - PCL solves a 3x3 float Jacobi SVD (Umeyama); here the closed 2-D form above in fp64.
 *  - PCL's behaviour when the cross-covariance vanishes (r == 0) is not restated.
 *  - The RANSAC threshold cloud_alignment.cpp:190 sets is taken to have no effect on an IterativeClosestPoint with no
 *    correspondence rejector installed (an assumption: PCL's text is not part of this project).
 *  - The reference's result is read from a float matrix; here from the fp64 state.
 *
 * POINT-TO-LINE METRIC (an addition, TBNAV_ICP_METRIC_LINE through tbnav_icp_set_metric; the default stays the point metric
 * above).  It has NO COUNTERPART IN THE REFERENCE, which only ever runs PCL's point-to-point ICP: this section is its whole
 * specification, restated in tests/icp_line_restatement.py and reproduced by the kernel bit for bit.  A source point is held
 * to the LINE through its nearest target point along the target cloud's tangent there, so it may slide along a wall: the
 * iteration converges in a few steps where the point metric converges linearly, it is not pulled along the wall towards
 * zero translation by the two scans sampling different points of it, and a direction the scan cannot see stays at the
 * initial guess or makes the alignment fail (DEGENERATE) instead of returning a confident wrong answer.
 * Unchanged from the point metric: the clouds (item 1), the initial guess (item 2), how a source point is transformed, the
 * nearest-neighbour search and its ties, the max_corr_dist gate, the summation order, the composition R <- R_inc * R,
 * t <- R_inc * t + t_inc, the stopping rules and their order (item 4), the result (item 5).  New, fp64 unless said, every
 * product and sum as parenthesised, no contraction:
 *  L1. Target normals, once per target cloud, with normal_window w (beams, 1..TBNAV_ICP_LINE_MAX_WINDOW, default 1) and
 *      normal_max_gap g (metres, > 0, default 0.25).  For a valid target beam i with point p_i: beam j is NEAR when it is
 *      valid and the fp32 d = dx*dx + dy*dy (dx = p_j.x - p_i.x, dy likewise, as in the search) has (double)d <= g*g.
 *      lo = the LOWEST near j in [max(0, i-w), i), or i when there is none; hi = the HIGHEST near j in
 *      (i, min(n_beams-1, i+w)], or i.  lo == hi: no normal.  Else tx = (double)p_hi.x - (double)p_lo.x, ty likewise,
 *      l = sqrt((tx*tx) + (ty*ty)); l == 0: no normal; else n_i = ((float)(-ty / l), (float)(tx / l)).  The gap keeps a
 *      normal from being drawn across a depth discontinuity (the beams on either side of it get one-sided normals).
 *  L2. Pairs: a source point is kept when its nearest target (the nearest of ALL target points, as in item 3) passes the
 *      distance gate AND has a normal.  Fewer than 3 kept: FAILED (TBNAV_ICP_NO_CORRESPONDENCES).
 *  L3. Sums per kept pair, a = the transformed source point (float, widened), b = the target, n = its normal (widened):
 *      ex = ax - bx, ey = ay - by, r = (nx*ex) + (ny*ey), j = (ax*ny) - (ay*nx); the count and, in the fixed order of item
 *      3, H00 += j*j, H01 += j*nx, H02 += j*ny, H11 += nx*nx, H12 += nx*ny, H22 += ny*ny, g0 += j*r, g1 += nx*r,
 *      g2 += ny*r, Sr += r*r.
 *  L4. Step: Gauss-Newton on sum (n . (R_inc a + t_inc - b))^2 linearised in the angle, unknowns (th, t_x, t_y), the
 *      translation eliminated first.  mse = Sr / n (it feeds the ABS / REL rules and info.mse, and is reported on DEGENERATE).
 *      tr = H11 + H22, det = (H11*H22) - (H12*H12); not det > K*(tr*tr): FAILED (TBNAV_ICP_DEGENERATE), K =
 *      TBNAV_ICP_LINE_MIN_COND.  v1 = ((H22*H01) - (H12*H02)) / det, v2 = ((H11*H02) - (H12*H01)) / det,
 *      dth = H00 - ((H01*v1) + (H02*v2)); not dth > K*H00: FAILED (TBNAV_ICP_DEGENERATE).
 *      th = -(g0 - ((v1*g1) + (v2*g2))) / dth; w1 = g1 + (H01*th), w2 = g2 + (H02*th);
 *      t_x = -((H22*w1) - (H12*w2)) / det, t_y = -((H11*w2) - (H12*w1)) / det.
 *      Rotation without a transcendental: u = 0.5*th, q = 1 + (u*u), c = (1 - (u*u)) / q, s = th / q: an exact rotation
 *      (c*c + s*s = 1) that agrees with th to third order and has the same fixed point th = 0.  The TRANSFORM rule uses this
 *      c and |t_inc|^2 = (t_x*t_x) + (t_y*t_y).
 *  K = 1e-6 is a design constant, not a measurement.  Where it sits: det / tr^2 (1/4 when the normals are spread evenly over
 *  all directions, 0 when they are all parallel) is 0.24-0.25 for the two rooms of tests/rbpf_cases.py, 0.048 for a 2 m wide
 *  corridor with 1 cm range noise, and 6.5e-11 for the same corridor without noise, where only the float rounding of the
 *  normals is left: a step taken on that throws the clouds apart.
 *  Divergences to know: the index window does not wrap from the last beam to beam 0 (the first and last w beams of a full
 *  turn get one-sided normals); normals are taken on the target cloud only; no robust weighting and no outlier rejection
 *  beyond the distance gate.
 *
 * CORRELATIVE SEARCH (an addition, off by default, tbnav_icp_set_search; csrc/icp_search.hip).  It has NO COUNTERPART IN THE
 * REFERENCE: this section is its whole specification, restated in tests/icp_search_restatement.py and reproduced by the kernels
 * EXACTLY (scores are integers: there is no tolerance anywhere).  The ICP above is a local method: from a guess that is wrong
 * by more than about half the correspondence gate it converges, ok = 1, onto a wrong answer (ROOM_BENCH of tests/rbpf_cases.py,
 * guess off by (0, 0.65, 0.65) m: ok after 9 iterations, 1.07 m off).  The search scores EVERY pose of a (theta, x, y) window
 * round the guess against a likelihood table of the target scan (Olson 2009; Cartographer's real-time correlative matcher)
 * and hands the best one to the ICP; it is exhaustive inside its window, so it has no basin.  All arithmetic is integer, or
 * fp64 with every product and sum as parenthesised and no contraction.
 *  S1. Parameters (tbnav_icp_search_params; defaults in brackets): resolution [0.05 m] the table's cell; half_extent E [4.0 m]
 *      half the table's side; sigma [0.05 m] and stamp_cells k [3, 1..8] the Gaussian stamp's width and half width in cells (k
 *      is an explicit integer on purpose: ceil(3 * 0.05 / 0.05) evaluates to 4 in doubles); lin_cells wl [6, 0..16] the window
 *      +-wl cells in x and y; ang_steps wa [20, 0..90] the window +-wa steps of ang_step [pi/180] radians; slack_q10
 *      [0, 0..1023] the selection slack in 1/1024; min_quality [0.5] the acceptance threshold.  n = 2 * ceil(E / resolution)
 *      cells per side, inv = 1.0 / resolution.  Required: resolution, E, sigma positive and finite, ang_step and min_quality
 *      finite, n >= 2 and n + 2*wl <= TBNAV_ICP_SEARCH_MAX_SIDE = 208 (the padded byte table then fits in LDS beside the source
 *      cells).  Anything else is TBNAV_ERR_INVALID_ARG and changes nothing.
 *  S2. Clouds: both are exactly item 1 above (the same code and beam table as the ICP's).
 *  S3. Stamp, on the host with glibc exp, (2k+1)^2 values of uint8, ox, oy in -k..k:
 *      stamp[oy][ox] = floor(255.0 * exp(-(d2 / (2.0 * (sigma*sigma)))) + 0.5), d2 = (double)(ox*ox + oy*oy) * (resolution*resolution).
 *  S4. Table, uint8 [n][n] indexed [iy][ix].  The cell of a target point p: ix = floor(((double)p.x + E) * inv), iy likewise.
 *      table[c] = the MAXIMUM of stamp[c - cell(p)] over the target points whose stamp covers c, 0 where none does (a maximum
 *      has no order).  A point whose cell is outside the table stamps the part that falls inside.
 *  S5. Candidates: na = 2*wa + 1 angles, nl = 2*wl + 1 offsets per axis.  theta_a = theta0 + (double)(ia - wa) * ang_step;
 *      (cos theta_a, sin theta_a) = (c, s) in double on the HOST with glibc, uploaded: no transcendental on the device.  A valid
 *      source point (sx, sy) (the doubles of its floats) under angle ia: ax = (((c * sx) - (s * sy)) + x0),
 *      ay = (((s * sx) + (c * sy)) + y0), x0 and y0 the DOUBLES of T_init; its base cell bx = floor((ax + E) * inv), by likewise.
 *      score[ia][iy][ix] = the sum over the valid source points of table[by + (iy - wl)][bx + (ix - wl)], a cell outside the
 *      table adding 0 (uint32).
 *  S6. Selection: best = the maximum score; thr = best - ((uint64)best * slack_q10 >> 10); among the candidates with
 *      score >= thr the one with the smallest D = (ia-wa)^2 + (iy-wl)^2 + (ix-wl)^2, then the lowest linear index
 *      (ia*nl + iy)*nl + ix.  slack_q10 = 0: the arg-max, ties going to the candidate nearest the guess.  candidates = the number
 *      of candidates with score >= thr.
 *  S7. Result: T = (theta0 + (double)(ia-wa)*ang_step, x0 + (double)(ix-wl)*resolution, y0 + (double)(iy-wl)*resolution), theta
 *      not wrapped; points = the valid source points; quality = (double)score / (255.0 * (double)points), 0 when points == 0;
 *      at_edge = 1 when the chosen index sits on the border of an axis whose half width is not zero;
 *      accepted = quality >= min_quality, and points > 0, and at least one target point.
 *  S8. In front of the ICP.  With the search on, tbnav_icp_match / _step / _step_batch (its realignment launches included)
 *      search every pair first, then run the ICP, with either metric, from T when accepted (T goes through item 2 like any
 *      guess) and from T_init UNCHANGED otherwise: a search that is not accepted gives the search-off result bit for bit.  The
 *      first tbnav_icp_step, which stores the scan, does not search.  tbnav_icp_step_batch stays n successive steps, bit for
 *      bit.  The search's result comes back to the host before the alignment is launched (the guess of item 2 is formed on the
 *      host, with glibc): one more stream synchronisation per launch.
 *  min_quality = 0.5 is a design constant, not a measurement.  Where it sits (a CPU prototype of this contract, the two rooms
 *  of tests/rbpf_cases.py, 1 cm range noise): a true match 0.76-0.90; the truth outside the window 0.14; the wrong room 0.42; a
 *  random cloud 0.09.  On the pairs above the search lands within one cell and 1 degree of the truth, and the ICP started
 *  from it ends 1.7 mm / 6.6 mrad off after 6 iterations.
 *  THE SHAPE OF THE SCORE VOLUME (an addition to the search, off by default, tbnav_icp_set_search_shape;
 *  csrc/icp_search_shape.hip; restated in tests/icp_search_shape_restatement.py, the integers reproduced exactly and the doubles
 *  by the same host arithmetic).  The search alone cannot tell an unobservable direction from an observable one: two noise-free
 *  scans of a corridor taken 10 cm apart along it are identical, the search overlays them and so moves the guess BACK by 10 cm.
 *  The score volume holds what is needed to see that: in a corridor the high scores form a ridge along it, in a room a compact
 *  blob.  With the shape on, the guess is kept along the direction(s) in which the chosen angle's scores are flat.
 *  F1. Parameters (tbnav_icp_search_shape_params; defaults in brackets): drop_q10 [256, 0..1023] how far below the chosen score
 *      a candidate still counts, in 1/1024 of it; flat_cells2 [2.0, finite and > 0] the second moment, in cells^2, above which a
 *      direction is flat.  Anything else is TBNAV_ERR_INVALID_ARG and changes nothing.
 *  F2. Weights, after S6 has chosen (ia, iy*, ix*) with score best: floor = best - (uint32)(((uint64)best * drop_q10) >> 10); for
 *      every candidate (iy, ix) of slice ia ONLY, all nl^2 of them: w = score > floor ? score - floor : 0.
 *  F3. Integer sums, dx = ix - wl, dy = iy - wl: S0 = sum w, Sx = sum w*dx, Sy = sum w*dy, Sxx = sum w*dx^2, Sxy = sum w*dx*dy,
 *      Syy = sum w*dy^2, cells = the number of candidates with w > 0.  Exact integers (int64 on the device: w < 2^20,
 *      dx^2 <= 2^8, at most 1089 cells, so every sum is below 2^39); no order is prescribed.
 *  F4. Moments, on the HOST in fp64, every product and sum as parenthesised, sqrt from glibc (S0 > 0):
 *      mx = Sx/S0, my = Sy/S0; a = (Sxx/S0) - (mx*mx), b = (Sxy/S0) - (mx*my), c = (Syy/S0) - (my*my);
 *      hd = 0.5*(a - c), h = sqrt((hd*hd) + (b*b)); l1 = (0.5*(a + c)) + h, l2 = (0.5*(a + c)) - h.
 *      Major axis, with no transcendental: v = hd >= 0 ? (hd + h, b) : (b, h - hd), n = sqrt((v.x*v.x) + (v.y*v.y)),
 *      e = n > 0 ? (v.x/n, v.y/n) : (1, 0).
 *  F5. Kind and result, d = ((double)(ix* - wl), (double)(iy* - wl)):
 *      kind 0 (compact: S0 == 0, or not l1 > flat_cells2): T is S7's, bit for bit.
 *      kind 1 (one flat direction: l1 > flat_cells2 and not l2 > flat_cells2): p = (d.x*e.x) + (d.y*e.y),
 *      d' = (d.x - (p*e.x), d.y - (p*e.y)); T.x = x0 + (d'.x * resolution), T.y = y0 + (d'.y * resolution).
 *      kind 2 (l2 > flat_cells2): d' = (0, 0), the translation is the guess's.
 *      The angle is S7's in every kind; quality, accepted, at_edge, candidates, ia / iy / ix are S7's, unchanged.  info->T is the
 *      shaped T, and that is what S8 hands to the ICP.
 *  F6. Record (tbnav_icp_search_shape): the six sums, l1, l2, e, cells, kind, T_raw = S7's T, computed = 1.  computed = 0 and
 *      everything else zero when the shape is off or no search ran.  With S0 == 0: l1 = l2 = ex = ey = 0.
 *  flat_cells2 = 2.0 is a design constant, not a measurement.  Where it sits (a CPU prototype of this contract, 360 beams, the
 *  default search parameters, 1 cm range noise): along a 2 m wide corridor l1 is 13.4-20.1 cells^2 (14.8 without noise) and
 *  across it l2 is 0.10-0.17; over 7 + 7 consecutive pairs in the two rooms of tests/rbpf_cases.py the largest l1 is 0.48 / 0.82,
 *  and 0.48 for ROOM_BENCH's 0.65 m bad guess with lin_cells = 14.  A uniform distribution over a window of +-2 cells has
 *  variance exactly 2.0: windows with lin_cells <= 2 can never be declared flat.  On the corridor pairs (robot 10 cm further
 *  along it, guess = truth) the search alone moves the guess 10-36 cm back and the line metric then ends 7.5-36 cm from the
 *  truth; with the shape it ends 0.8-3.9 mm from it, and a guess also 15 cm and 0.05 rad off ACROSS the corridor ends 1.3 mm off
 *  (32 mm without the search, 128 mm with the search alone): the correction across the corridor is kept.
 *  KNOWN LIMITS.  A guess that is wrong ALONG an unobserved direction cannot be repaired by anyone: the shape only keeps the
 *  search from making it worse.  Only the translation is examined, and only in the chosen angle's slice: an angle the scan does
 *  not determine (a round room) is not detected.  The point metric still pulls the two scans of a corridor together afterwards;
 *  the line metric is the one that keeps what the shape kept.  Translation accuracy of the search is one cell: the ICP behind
 *  it is what refines it.
 *  WIDE WINDOW (an addition to the search, off by default, tbnav_icp_set_search_wide; csrc/icp_search_wide.hip; restated in
 *  tests/icp_search_wide_restatement.py, reproduced exactly).  S1 caps the window at +-16 cells because icp_search_score keeps the
 *  whole padded table in LDS.  A guess further off than that (a long wheel slip, a robot that was picked up) is outside every
 *  window of the first stage: the search is rejected and the ICP starts from the bad guess.  The wide window is a SECOND STAGE
 *  that scores up to +-64 cells and +-180 steps, tiled over workgroups, and is charged only when it is needed.  All arithmetic is
 *  S5-S7's: integer, or fp64 with every product and sum as parenthesised and no contraction.
 *  W1. Parameters (tbnav_icp_search_wide_params; defaults in brackets): lin_cells W [48, 1..TBNAV_ICP_SEARCH_WIDE_MAX_LIN = 64];
 *      ang_steps A [45, 0..TBNAV_ICP_SEARCH_WIDE_MAX_ANG = 180]; when [TBNAV_ICP_WIDE_ON_REJECT = 0; TBNAV_ICP_WIDE_ON_REJECT_OR_EDGE
 *      = 1, TBNAV_ICP_WIDE_ALWAYS = 2]; one reserved int32.  Everything else is the first stage's tbnav_icp_search_params:
 *      resolution, half_extent, sigma, stamp_cells, ang_step, slack_q10, min_quality.  Three conditions hold against the search
 *      parameters the handle holds (the defaults while the search is off): W >= lin_cells, A >= ang_steps, and the table side
 *      n <= TBNAV_ICP_SEARCH_WIDE_MAX_TABLE = 176.  The wide window then contains the first, so its best score is never below the
 *      first stage's, and a tile of up to 33 translations per axis fits in the LDS the first stage's scoring kernel uses.
 *      tbnav_icp_set_search_wide with a bad field or a violated condition is TBNAV_ERR_INVALID_ARG and changes nothing;
 *      tbnav_icp_set_search with parameters that violate a condition while the wide stage is on is the same (params == NULL
 *      stands for the defaults there); with the wide stage off tbnav_icp_set_search is unchanged.  The defaults are design
 *      constants, not measurements: +-2.4 m and +-45 degrees.
 *  W2. First stage: S1-S7 run unchanged and give the record `first`.  With when = ALWAYS the first stage is not run:
 *      first.searched = 0 and every other field 0.
 *  W3. The wide stage runs when when = ALWAYS, or first.accepted = 0, or when = ON_REJECT_OR_EDGE and first.at_edge = 1.
 *  W4. Wide stage: S5, S6 and S7 with wl := W and wa := A, on the same table (the target is stamped once per pair, not once per
 *      stage), the same clouds and the same doubles T_init.  theta_a = theta0 + (double)(ia - A) * ang_step, its cosine and sine
 *      from the host's glibc.  ia, iy, ix, at_edge, candidates, quality and accepted are S6 / S7's over the wide window.  With
 *      A = 180 and a step of pi/180 the first and the last angle are the same direction: S6's lowest linear index breaks the tie.
 *  W5. Outcome: the wide stage's record if it ran, `first` otherwise.  S8 reads "the outcome" where it reads "the search":
 *      tbnav_icp_match, _step, _step_batch (its realignment launches included) and the stateless tbnav_icp_search and
 *      tbnav_icp_search_with_shape.  tbnav_icp_last_search returns the outcome; tbnav_icp_last_search_wide returns
 *      tbnav_icp_search_wide_info (first, ran) with the same lifetime.  A wide stage that is on but did not run leaves every
 *      result equal, bit for bit, to the same handle with the wide stage off.  tbnav_icp_step_batch stays n successive steps.
 *      tbnav_icp_search_scores and tbnav_icp_search_table are the first stage's hooks and ignore the wide stage.
 *  W6. Shape: F1-F6 apply to the stage that produced the outcome, with wl := W where that is the wide stage.  F3's sums stay
 *      exact in int64: w < 2^20, dx^2 <= 2^12 and at most 129^2 cells put every sum below 2^47.  CPU evidence (corridor pair 3
 *      of tests/test_icp_search_shape_restatement.py, guesses (0.45, 0.10, 0.15) and (0.45, 0.10, 0.6), first stage rejected
 *      with q 0.50 and 0.11): at W = 32 and W = 64 with A = 30 the raw wide choice overlays the scans and moves the 10 cm along
 *      the corridor back to 0; the shape returns kind 1 with l1 = 234 / 260 and l2 = 0.06 and keeps x at the guess's 0.10; the
 *      line metric then ends 32 mm off along the corridor, against 128 mm from the raw choice.
 *  W7. Limits: n_beams <= TBNAV_ICP_MAX_BEAMS, as for the first stage.  The wide stage is stored but idle while the search is
 *      off; the stateless entries honour it anyway, as they do the shape.  tbnav_icp_set_search_wide(h, NULL) turns it off and
 *      resets its parameters; tbnav_icp_set_search(h, NULL) leaves it stored.  A new handle has it off.
 *  W8. Test hook tbnav_icp_search_wide_scores: stateless, the wide stage alone whatever `when` says, with the handle's search and
 *      wide parameters (the defaults while they are off; the shape when the handle has it on); scores may be NULL, otherwise
 *      [2A+1][2W+1][2W+1].
 *  MAP SEARCH (an addition to the search, tbnav_icp_search_map; csrc/icp_search_map.hip; restated in
 *  tests/icp_search_map_restatement.py, reproduced exactly).  The search above scores a window of poses against a table of THE
 *  PREVIOUS SCAN: it repairs one slipped scan, not a pose that has drifted over many scans, a robot that was picked up, or a filter
 *  restarted in a map it already holds, where the previous scan is as wrong as the guess.  The map search forms the table from the
 *  occupied cells of a filter particle's MAP (tbnav_rbpf.h) instead, on the device, and runs everything behind the table unchanged.
 *  M1. Handles: an ICP handle h and a filter handle pf, on one device (else TBNAV_ERR_UNSUPPORTED; a member of a sharded group is
 *      TBNAV_ERR_UNSUPPORTED too).  The search parameters are h's (the defaults while its search is off, as for the other
 *      stateless entries); their resolution must equal the filter's as doubles, else TBNAV_ERR_INVALID_ARG (a filter's map
 *      is always square: tbnav_rbpf_create refuses another).  Order: arguments, parameters and particles are looked
 *      at first (INVALID_ARG), then device and group (UNSUPPORTED), then the guesses (M3, OUT_OF_WORLD).  The beam geometry and Trs that form the cloud are h's own (item 1): making them the filter's is the
 *      caller's business.  particle is a slot of the filter or TBNAV_ICP_MAP_BEST_PARTICLE (-1): the arg-max of the weights found
 *      on the device by tbnav_rbpf_best_state's rule (strict >, the first wins), as tbnav_nav.h G8 does.  Anything rejected
 *      changes nothing: neither the filter, nor h's parameters, stored scan or last records.
 *  M2. Occupied: a map cell is occupied when its bit in the particle's tiles is set (G8's definition, whatever distance-field mode
 *      the filter runs in).  The cell (ci, cj) of a world position is G1's: ci = (int)floor((x - xmin) * inv), inv = 1.0 / resolution.
 *  M3. Frame: T_init = (theta0, x0, y0) is the robot's guessed pose in the WORLD.  (cx, cy) = M2's cell of (x0, y0); a guess that
 *      is not finite (any of the three) or whose cell is outside the map is TBNAV_ERR_OUT_OF_WORLD.  h2 = n / 2 with S1's n.  The
 *      table's origin is o = (xmin + (double)cx * resolution, ymin + (double)cy * resolution).  Table cell [iy][ix] IS map cell
 *      (cx - h2 + ix, cy - h2 + iy); cells outside the map are not occupied.  E' = (double)h2 * resolution takes the place of S1's E
 *      in S5: with a half_extent that is not a whole number of cells the table's cells would otherwise not be the map's.
 *  M4. Table: table[iy][ix] = the maximum of stamp[my - (cy - h2 + iy) + k][mx - (cx - h2 + ix) + k] over the occupied map cells
 *      (mx, my) with both offsets in -k..k, 0 where there is none; stamp is S3's.  This is S4's table of the occupied cells'
 *      centres.  tgt_points = the number of occupied cells inside the n x n window itself.  (S3's stamp depends on ox^2 + oy^2 only
 *      and never rises with it: the maximum is the stamp at the least squared distance.  The host checks that property for the
 *      parameters in force and answers TBNAV_ERR_UNSUPPORTED should it ever fail.)
 *  M5. Scoring, selection, result: S5-S7 run unchanged on that table with the local guess (theta0, (x0 - o.x), (y0 - o.y)) (two
 *      fp64 subtractions on the host) and E := E'.  S7's T is formed from the WORLD T_init: x0 + (double)(ix - wl) * resolution
 *      already is the world pose.  accepted reads tgt_points > 0 where S7 reads "at least one target point".
 *  M6. Shape and wide stage: F1-F6 and W1-W8 apply as they stand, "the table" being M4's.  W1's limits are unchanged (n <= 176 with
 *      the wide stage on); `when` keeps its meaning.
 *  M7. Batch: one scan, n >= 1 pairs (particle_i, T_init_i), independent, each equal to the single call bit for bit: several
 *      hypotheses against one particle's map, or every particle against its own.  One bad pair rejects the call before any launch.
 *  M8. Ordering and state: the table kernel runs behind whatever the filter handle has in flight (an event between the two
 *      streams, no host synchronisation) and the scoring behind the table; the call returns with the result on the host.  The
 *      filter is only read.  h's stored scan (tbnav_icp_step) is neither read nor written.  tbnav_icp_last_search,
 *      _last_search_shape and _last_search_wide report this search (of a batch: the last pair's).
 *  M9. Known limits.  Accuracy is one cell and one angle step: the refinement below one cell against the same map is tbnav_icp_align_map (MAP
 *      ALIGNMENT, A1-A11 below), which a caller runs from info->T; the search itself does not run it.  Points further than E' from the guess's cell
 *      add nothing, as in the scan search.  Unknown cells and free cells both score 0: the search has no free-space penalty; whether a
 *      beam passes through a wall or ends in space the map knows to be free is asked by tbnav_icp_verify_map (MAP CHECK, V1-V10 below).
 *      min_quality = 0.5 was set for scan pairs; over a WIDE window against a map it does not separate a true match from a wrong
 *      room (tests/icp_search_map_cases.py, BEHAVIOUR: the restatement on maps drawn by the oracle's GridMapper from 12 / 20 scans
 *      of the two rooms of tests/rbpf_cases.py: true matches at +-48 cells and +-45 steps 0.872 and 0.984, a scan of the other room
 *      0.557, ACCEPTED; at +-14 cells the other room is 0.402, rejected): a caller who searches wide against a map should raise
 *      min_quality.  The other side of the same coin, from the same table: the table stands round the GUESS's cell, so a guess
 *      2.5 m off in a 6 x 5 m room leaves two walls outside it; the pose is found to the cell and REJECTED at 0.417, because quality
 *      divides by all valid points.  A caller far off should look at at_edge and the pose, or search again from info->T.
 *      The default is unchanged.  The map search is not wired into
 *      tbnav_icp_step / _match nor into bmapping::ParticleFilter::SLAM: a caller composes it.
 *  KERNEL (csrc/icp_search_map.hip): icp_search_table_from_occ, one workgroup of 256 threads per (32 x 32 tile of the table, pair):
 *  the occupancy words of the tile's map rows and 8 either side, read through the particle's tile table (tile id 0, tiles outside
 *  the map and a ragged last tile read as empty) and funnel-shifted to the table's origin; per cell the nearest set bit by rows
 *  outwards (clz / ffs, stopping when dr^2 reaches the best) and one look into a value-by-squared-distance table; the tile
 *  transposed through LDS and written, border of wl zero cells included, in icp_search_table's padded layout.  Integers only, no
 *  atomic but the count of tgt_points.
 *  KERNELS (csrc/icp_search_wide.hip): icp_search_wide_score, one workgroup of 256 threads per (translation tile, angle, pair):
 *  a tile is up to 33 x 33 translations; the base cells are shifted by the tile's first offset, so the workgroup needs the table
 *  with tile - 1 zero cells on its high side only (side <= 208, read from the first stage's padded table in global memory);
 *  icp_search_wide_select, one workgroup per pair, reduces the tiles x angles 64-bit keys (score, then the inverted 39-bit rank
 *  D << 23 | linear index).  slack_q10 > 0 scores a second time against thr; the shape is a third pass over the chosen angle's
 *  tiles, one partial record per tile that the host adds.  In a batch the wide stage runs behind the synchronisation that brings
 *  a chunk's first-stage records back, for the pairs W3 names, and costs one more synchronisation only when there is one.
 *  KERNELS (csrc/icp_search.hip): icp_search_table, one workgroup per pair, stamps the target into a byte table in LDS (a
 *  compare-and-swap maximum on the byte's dword) and writes it padded with wl zero cells on every side; icp_search_score, one
 *  workgroup of 256 threads per (pair, angle), keeps the padded table and its angle's base cells in LDS, each thread owning
 *  translations and walking the points (base cells outside the table, whose window is only partly inside, take a
 *  bounds-tested path), and reduces one 64-bit key (score high, inverted rank low) per workgroup; icp_search_select reduces
 *  the na keys.  slack_q10 > 0 scores a second time against thr.  n_beams <= TBNAV_ICP_MAX_BEAMS with either metric.
 *  icp_search_shape (csrc/icp_search_shape.hip), one workgroup per pair behind the final icp_search_select and only when the
 *  shape is asked for, scores the chosen angle once more in the same way and reduces the integers of F3; its 64-byte record
 *  comes back in the synchronisation that brings the selection back: no further synchronisation.
 *  GLOBAL SEARCH (an addition, tbnav_icp_localize_map; csrc/icp_global.hip; restated in tests/icp_global_restatement.py, reproduced
 *  exactly).  The map search scores a window round a guess: a table of at most 176 / 208 cells a side, +-64 cells and +-180 steps.
 *  The global search takes NO guess: it scores every heading at every cell of a particle's map, and prunes with an upper bound
 *  taken from a max-pooled copy of the likelihood map (Olson 2009; Cartographer's fast correlative matcher).  The bound is exact,
 *  so the result is the exhaustive search's.  All arithmetic is integer but for L3's offsets.
 *  L1. Handles and parameters.  An ICP handle h and a filter handle pf as in M1: one device, no member of a sharded group, and M1's
 *      order of the checks (arguments, parameters and the particle: INVALID_ARG; then device, group and the limits below:
 *      UNSUPPORTED).  The cloud's beam geometry and Trs are h's (item 1); stamp_cells, sigma and resolution are h's search parameters
 *      (the defaults while its search is off); the resolution must equal the filter's as doubles.  particle is a slot or
 *      TBNAV_ICP_MAP_BEST_PARTICLE.  side = the map's side <= TBNAV_ICP_GLOBAL_MAX_SIDE = 2048, a larger one is
 *      TBNAV_ERR_UNSUPPORTED (a candidate's linear index then fits in 32 bits: 720 * 2048^2 < 2^32).
 *      tbnav_icp_global_params (defaults in brackets): ang_count NA [360, 1..TBNAV_ICP_GLOBAL_MAX_ANG = 720]; ang_step [pi/180,
 *      finite]; pool_log2 q [3, 1..5], s = 2^q; region[4] = (tx0, ty0, tx1, ty1), inclusive cells [all -1: the whole map], otherwise
 *      0 <= tx0 <= tx1 < side and likewise for y, w = tx1 - tx0 + 1, h = ty1 - ty0 + 1; min_quality [0.5, finite]; one reserved
 *      int32 that must be 0.  NULL params are the defaults.  A bad field is TBNAV_ERR_INVALID_ARG.  More than 2^26 blocks (L5) is
 *      TBNAV_ERR_UNSUPPORTED.  n_beams is 1..TBNAV_ICP_MAX_BEAMS.  Anything rejected changes nothing; the filter is only ever
 *      read; h's stored scan, its parameters and the last records of the other searches are untouched by any call of this section.
 *  L2. Likelihood map.  lik(ci, cj), a uint8 for every map cell, is M4's value with the map cell in the table cell's place: the
 *      maximum of stamp[mj - cj + k][mi - ci + k] (S3's stamp) over the occupied cells (mi, mj) (M2) with both offsets in -k..k, 0
 *      where there is none.  lik is 0 for every cell outside the map.  The host's check that the stamp never rises with the squared
 *      distance, and its TBNAV_ERR_UNSUPPORTED, are M4's.  occupied = the number of occupied cells of the map.
 *  L3. Candidates.  Heading ia in 0..NA-1: theta = (double)ia * ang_step, its cosine and sine (c, s) from the host's glibc, uploaded
 *      (as in S5).  The robot stands at the CENTRE of map cell (tx, ty) of the region.  For a valid source point (sx, sy) (the
 *      doubles of its floats) the cell offset is taken once per heading: vx = ((((c * sx) - (s * sy))) * inv) + 0.5,
 *      vy = ((((s * sx) + (c * sy))) * inv) + 0.5, fp64 with no contraction, inv = 1.0 / resolution; ox = (int)floor(vx),
 *      oy = (int)floor(vy).  A point with vx or vy not within +-65536 (a NaN included) adds nothing at that heading (S5's guard).
 *      score(ia, tx, ty) = the sum over the valid points of lik(tx + ox, ty + oy), a uint32.  The offsets do not depend on
 *      (tx, ty): that is what makes L5's bound exact.
 *  L4. Result.  The maximum score over all candidates, ties going to the lowest linear index (ia * side + tx) * side + ty.
 *      T = (theta, xmin + ((double)tx + 0.5) * resolution, ymin + ((double)ty + 0.5) * resolution), theta not wrapped.  points = the
 *      valid source points; quality = (double)score / (255.0 * (double)points), 0 with no point; accepted = quality >= min_quality
 *      and points > 0 and occupied > 0.  With points = 0 or occupied = 0 every score is 0: the result is the region's first
 *      candidate (ia = 0, tx0, ty0) with accepted = 0.
 *  L5. Blocks and bounds.  Blocks of s x s cells tile the region from (tx0, ty0); the last ones may be ragged.  nbx = ceil(w / s),
 *      nby = ceil(h / s), blocks = NA * nbx * nby.  pool(i, j) = the maximum over 0 <= a, b < s of lik(i + a, j + b), for any
 *      integers i, j: the window FORWARD of the cell.  bound(ia, Bx, By) = the sum over the valid points of
 *      pool(tx0 + Bx * s + ox, ty0 + By * s + oy) (the guarded points of L3 adding nothing).  bound >= the score of every
 *      candidate of the block; a ragged block's pool reaches past the region, which only raises the bound.
 *  L6. What the search may skip: a block only if its bound is < a score some candidate has actually attained.  A block whose bound
 *      EQUALS that score may hold the answer by L4's index rule, so it is refined.  How seeds are chosen, how many rounds run and
 *      how survivors are listed is the implementation's; the result is L4's whatever they are.  refined_blocks (the blocks whose
 *      candidates were all scored) and rounds (the refinement launches) are reported.
 *  L7. Record tbnav_icp_global_info: searched, accepted, T[3], ia, tx, ty, score, points, occupied, quality, blocks, refined_blocks
 *      (int64 both), rounds.  searched = 0 and everything else 0 before the first call.
 *  L8. Ordering: M8's.  The kernels run behind whatever the filter's stream has in flight, through an event, with no host
 *      synchronisation of that stream; the call returns with the record on the host.
 *  L9. Entries: tbnav_icp_localize_map; tbnav_icp_localize_map_timed (the same call, its stages timed by events); tbnav_icp_last_global; tbnav_icp_last_global_kernels (the last call's kernels by the names a
 *      profiler prints, ';'-separated, "" before the first call).  Test hooks, stateless (the last record and the kernel names stay):
 *      tbnav_icp_localize_map_field (lik [side][side] indexed [ci][cj]; pool [side + s - 1][side + s - 1] indexed
 *      [i + s - 1][j + s - 1] for i, j in -(s - 1)..side - 1: the s - 1 rows and columns before cell 0 included; occupied);
 *      tbnav_icp_localize_map_bounds (uint32 [NA][nbx][nby]); tbnav_icp_localize_map_scores (EVERY candidate's score,
 *      uint32 [NA][w][h] indexed [ia][tx - tx0][ty - ty0], computed by the refinement kernel run over all blocks;
 *      TBNAV_ERR_UNSUPPORTED above 2^24 candidates).
 *  L10. Not built: a free-space penalty or a restriction to FREE cells inside the search (M9's wrong-room finding applies unchanged; a
 *      caller checks the pose it gets with tbnav_icp_verify_map, MAP CHECK V1-V10, which refuses that wrong room); (several
 *      hypotheses, for a symmetric building that has several equal answers, are tbnav_icp_localize_map_hyp, HYPOTHESES H1-H10);
 *      sub-cell or sub-step refinement inside this call (a caller runs tbnav_icp_align_map, MAP ALIGNMENT A1-A11, from T); seeding the
 *      filter's particles from the result; batches of scans; sharded filters; more than one level of pooling in the contract (an
 *      implementation may use more inside, L6).
 *  KERNELS (csrc/icp_global.hip).  icp_global_field, one workgroup of 256 threads per 32 x 32 map tile: icp_search_table_from_occ's
 *  staged rows and nearest-set-bit search (icp_search_device.hpp: occ_row_window, nearest_occ_d2) with the window at the tile itself;
 *  lik goes into a byte map [P][P], P = side + 2 * 32 rounded up to 64, cell (ci, cj) at [ci + 32][cj + 32], the margin zero, so that
 *  a gather needs a clamp of its coordinates (one v_med3 each) and no bounds test; occupied is one integer atomic add per tile.
 *  icp_global_pool: the s x s forward sliding maximum of that map, rows then columns through LDS, into a second map of the same
 *  layout.  icp_global_offsets, one workgroup per heading: L3's (ox, oy) of the points that can add anything, packed as two int16
 *  and compacted in no order (a sum of integers has none), with their count; points.  icp_global_bound, one workgroup per (heading,
 *  4 x 64 blocks): the heading's offsets in LDS, lanes along By (ty is the map's fast index, so a wave's gathers for one point fall
 *  in one row of the pooled map); it also leaves the largest bound.  icp_global_hist: 1024 bins over 0..the largest bound, from which
 *  the host takes the least bound that still leaves 16 seeds.  icp_global_list: the blocks with lo <= bound < hi into a list
 *  through one slot counter (round 1: the seeds; round 2: lo = the best score the seeds attained, hi = the seeds' least bound).
 *  icp_global_refine, one workgroup per listed block, scores its s^2 candidates against lik and settles maximum and tie with one
 *  64-bit atomicMax of (score << 32 | ~linear index) per wave; a block whose bound is 0 holds only zeros and is settled by its
 *  first candidate without a gather.  No workgroup waits for another; every loop is bounded by the points, the tile or s; a round is
 *  a launch and the host reads one small record per round: at most two rounds.
 *  HYPOTHESES (an addition, tbnav_icp_localize_map_hyp; csrc/icp_hyp.hip behind csrc/icp_global.hip; restated in
 *  tests/icp_hyp_restatement.py, reproduced exactly).  The global search returns ONE pose, the maximum, ties going to the lowest index;
 *  a symmetric building has several equal answers, and score alone cannot choose between a true pose and a wrong room (M9).  This entry
 *  returns the global search's separated peaks: every candidate at or above a floor that no candidate of its window beats, in order.
 *  A caller aligns and checks each of them (tbnav_icp_align_map_batch, tbnav_icp_verify_map_batch) and learns which survive, and
 *  whether more than one does.  It is opt-in; no other entry calls it and no other entry's record is touched.  Integers only.
 *  H1. Handles, parameters, checks.  The handles, tbnav_icp_global_params, the particle and the order of the checks are L1's, unchanged.
 *      tbnav_icp_hyp_params (defaults in brackets): max_hyp K [8, 1..TBNAV_ICP_HYP_MAX = 64]; floor_q10 f [768, 1..1024]; sep_cells
 *      [8, 0..64]; sep_steps [10, 0..TBNAV_ICP_GLOBAL_MAX_ANG]; wrap [1, 0 | 1]; one reserved int32 that must be 0.  NULL is the
 *      defaults; a bad field is TBNAV_ERR_INVALID_ARG.  Bins: Ba = sep_steps + 1, B = sep_cells + 1, bins = ceil(NA / Ba) *
 *      ceil(w / B) * ceil(h / B); more than TBNAV_ICP_HYP_MAX_BINS = 2^22 bins is TBNAV_ERR_UNSUPPORTED (behind L1's own limits).
 *      Anything rejected changes nothing.
 *  H2. Scores and the floor.  Candidates, scores and the linear index are L3 / L4's.  key(c) = (score << 32) | ~index: a greater key is
 *      a higher score, then a lower index.  best = L4's maximum score; the floor t = (best * f + 1023) >> 10 in 64-bit integers.  With
 *      best = 0 (no valid point, or an empty map) the result is empty (n = 0), not an error; floor_score, floor_blocks, candidates and
 *      n_peaks are 0 then.
 *  H3. Window.  c' lies in c's window when |tx' - tx| <= sep_cells, |ty' - ty| <= sep_cells and d(ia', ia) <= sep_steps;
 *      d = |ia' - ia| when wrap = 0, and min(|ia' - ia|, NA - |ia' - ia|) when wrap = 1.  The relation is symmetric.  Only the region's
 *      candidates exist.
 *  H4. Peak: a candidate with score >= t whose key is the greatest among all candidates in its window.  A candidate with a greater key
 *      has score >= its score >= t, so only candidates at or above the floor can suppress one; a suppressor need not be a peak itself.
 *      No two peaks lie in each other's window.  A plateau of equal scores has one peak per window-connected run: the lowest index.
 *      L4's result is always a peak.
 *  H5. Result: the peaks in descending key order, the first n = min(K, n_peaks) of them; hypothesis 0 is L4's answer.  Per hypothesis
 *      (tbnav_icp_hypothesis): T[3] (L4's formula), quality, score, ia, tx, ty, accepted (L4's rule with gp.min_quality).
 *  H6. What may be skipped, and the limits.  A block may be skipped only if its bound is < t.  How best is found, how blocks are listed
 *      and how peaks are found is the implementation's.  More than TBNAV_ICP_HYP_MAX_REFINE = 2^18 blocks with bound >= t, or (looked
 *      at second) more than TBNAV_ICP_HYP_MAX_CANDIDATES = 2^20 candidates with score >= t, is TBNAV_ERR_UNSUPPORTED with nothing
 *      changed.  Both are functions of L5's bound volume and L3's score volume alone.
 *  H7. Record tbnav_icp_hyp_info: searched, n, n_peaks, best_score, floor_score, points, occupied, blocks, floor_blocks (bound >= t),
 *      refined_blocks (the distinct blocks whose candidates were all scored: floor_blocks <= refined_blocks <= blocks), candidates
 *      (score >= t), rounds (the scoring launches).  All 0 before the first call.
 *  H8. Ordering: L8's.
 *  H9. Entries: tbnav_icp_default_hyp_params; tbnav_icp_localize_map_hyp (cap < 1 is INVALID_ARG; otherwise the call fills
 *      min(cap, n) hypotheses and reports n); tbnav_icp_last_hyp; tbnav_icp_last_hyp_kernels (';'-separated names as a profiler prints
 *      them, "" before the first call).  Test hook, stateless: tbnav_icp_localize_map_hyp_candidates, every candidate with score >= t
 *      in ascending index order as (index uint32, score uint32, peak uint8) and their count (the host sorts: the device's order is
 *      free).
 *  H10. Not built: a floor relative to anything but the best score; sub-cell refinement inside the call; batches of scans; sharded
 *      filters; seeding the filter's particles from the survivors.
 *  KERNELS (csrc/icp_hyp.hip), behind the global search's own (which find best) and one more icp_global_list with lo = t:
 *  icp_hyp_collect, one workgroup per listed block in icp_global_refine's shape (the heading's offsets in LDS, lanes over the block's
 *  cells): every candidate with score >= t is appended to a list of keys, one integer atomic add per wave (ballot, count, the lanes
 *  take consecutive slots), and folded into its bin of Ba x B x B candidates with a 64-bit atomicMax.  icp_hyp_knock, one lane per
 *  listed candidate: for every bin that can hold a candidate of its window (3 x 3 spatial bins times the angular bins its headings
 *  fall in, modulo NA with wrap) it reads the bin's winner and, when that lies inside the window with a lesser key, clears the winner's
 *  alive flag.  A bin is no wider than a window's half extent + 1, so a peak is its bin's winner, and every candidate of a winner's
 *  window lies in those bins: the alive winners are exactly H4's peaks.  Winners compared only with winners would NOT be: a
 *  neighbouring bin's winner can lie outside the window while a lesser member lies inside and still beats the candidate.
 *  icp_hyp_select, one workgroup: flags, counts and compacts the peaks and leaves the first K in key order.  One read-back for all
 *  three; no workgroup waits for another.
 *  MAP ALIGNMENT (an addition, tbnav_icp_align_map; csrc/icp_align_map.hip; restated in tests/icp_align_map_restatement.py, reproduced
 *  bit for bit).  It has NO COUNTERPART IN THE REFERENCE: this section is its whole specification.  The map search and the global
 *  search stop at one cell and one angle step; the ICP above aligns to the PREVIOUS SCAN, which after a relocalisation is as wrong as
 *  the guess.  This is the local, metric alignment of one scan to a particle's map: the last link of global search -> window search ->
 *  alignment.  It is opt-in and stateless; no other entry calls it.  A point-to-line step (L3, L4) against a line fitted to the
 *  occupied cells round the nearest one (the idea of the normal-distributions transform).  What it must not be (CPU prototype, bench
 *  room, maps rasterised from 12 synthetic scans at 0.05 m, starts within half a cell and half a degree): ICP against the CENTRE of
 *  the nearest occupied cell ends 34.7 mm off from starts 19.9 mm off, because a wall on a cell border is drawn two cells thick and
 *  each row of centres is a stable fixed point; Gauss-Newton on the interpolated table M4 has the same band.  Arithmetic is integer,
 *  or fp64 with every product and sum as parenthesised and no contraction; no transcendental, and no device sqrt or division but the
 *  correctly rounded fp64 ones.
 *  A1. Handles, particle, order of the checks.  An ICP handle h and a filter handle pf on one device (else TBNAV_ERR_UNSUPPORTED; a
 *      member of a sharded group is TBNAV_ERR_UNSUPPORTED too).  Order: arguments, parameters and particles first (INVALID_ARG), then
 *      device and group (UNSUPPORTED), then the guesses (A3, OUT_OF_WORLD).  particle is a slot or TBNAV_ICP_MAP_BEST_PARTICLE (M1's
 *      arg-max).  The cloud's beam geometry and Trs are h's (item 1); max_iter, transform_eps and fitness_eps are h's (item 4);
 *      max_corr_dist and h's search parameters take no part: the grid (xmin, ymin, resolution, side) is the filter's.  n_beams is
 *      1..TBNAV_ICP_MAX_BEAMS.  Anything rejected changes nothing: not the filter, not h's parameters, its stored scan or any last
 *      record.  An accepted call reads the filter, leaves h's stored scan and every last record of the searches alone, and changes
 *      only what tbnav_icp_last_align_map_kernel reports.
 *  A1a. Parameters (tbnav_icp_align_map_params; defaults in brackets; NULL: the defaults; a bad field is TBNAV_ERR_INVALID_ARG):
 *      half_cells H [128, 8..TBNAV_ICP_ALIGN_MAP_MAX_HALF = 256]; gate_cells G [10, 1..16]; feature_cells w [2, 1..4]; max_flatness f
 *      [0.25, finite, 0 <= f < 1]; one reserved int32 that must be 0.
 *  A2. Occupied and cells: M2 as it stands (the occupancy bit; ci = (int)floor((x - xmin) * inv), inv = 1.0 / resolution).
 *  A3. Window.  (cx, cy) = A2's cell of (x0, y0) of T_init, a WORLD pose; a T_init that is not finite (any of the three) or whose cell
 *      is outside the map is TBNAV_ERR_OUT_OF_WORLD.  The window is the 2H x 2H cells (cx - H .. cx + H - 1, cy - H .. cy + H - 1).
 *      For everything below an occupied cell EXISTS only if it lies inside both the window and the map.  The window stays where
 *      T_init put it for all iterations.
 *  A4. Feature of an occupied cell m = (mi, mj), over the occupied cells q (A3) with |qi - mi| <= w and |qj - mj| <= w, m included.
 *      Integers, d = q - m: n, sx = sum di, sy = sum dj, sxx = sum di*di, sxy = sum di*dj, syy = sum dj*dj; a = n*sxx - sx*sx,
 *      c = n*syy - sy*sy, b = n*sxy - sx*sy.  Centroid: bx = xmin + (((double)mi + 0.5) + ((double)sx / (double)n)) * resolution, by
 *      likewise with mj, sy, ymin.  Eigenvalues: hd = 0.5 * (double)(a - c), dd = sqrt((hd*hd) + ((double)b*(double)b)),
 *      lmin = (0.5 * (double)(a + c)) - dd, lmax = (0.5 * (double)(a + c)) + dd.  The cell HAS A NORMAL when n >= 3 and lmax > 0 and
 *      lmin <= f * lmax.  Direction: b != 0: v = ((double)b, lmin - (double)a); b == 0: v = (0, 1) when a >= c, else (1, 0);
 *      l = sqrt((vx*vx) + (vy*vy)); normal = ((float)(vx / l), (float)(vy / l)).  f is a design constant, not a measurement: it keeps
 *      blobs and the inside of corners from handing out a direction.
 *  A5. Pairing, each iteration.  A source point goes to a exactly as in item 3, from the float-rounded guess of item 2 held in fp64.
 *      Its home cell (hi, hj) is A2's cell of the doubles of a (the floor is compared as a double: a point that is not a number has
 *      no home); a point whose home is outside the window has no pair.  Its target cell is the occupied cell (A3) with |mi - hi| <= G
 *      and |mj - hj| <= G that minimises the integer D = (mi - hi)^2 + (mj - hj)^2; ties go to the lowest mi, then the lowest mj.
 *      The pair is kept when D <= G*G and the target cell has a normal (a cell inside the box and outside the disc is the target and
 *      is dropped).
 *  A6. Sums, step, composition, stopping: L3 and L4 as they stand with b := the centroid (bx, by) in doubles and n := the doubles of
 *      the float normal; item 3's fixed summation order (thread t of 256 adds the kept pairs of beams t, t + 256, ... in increasing
 *      order, then the tree); fewer than 3 kept pairs: TBNAV_ICP_NO_CORRESPONDENCES; L4's two DEGENERATE tests with the same K;
 *      composition and item 4's rules and their order unchanged.
 *  A7. Result: tbnav_icp_info as for the other alignments (criterion, iterations, correspondences and mse of the last iteration) and
 *      ok (1 when converged); T is item 5's, in the WORLD.  On a failure T_out is T_init's three doubles UNCHANGED and ok = 0: this
 *      differs from item 5, whose failure is (0, 0, 0), because here T is a world pose and the guess is the best pose known.
 *  A8. Batch: one scan and n >= 1 pairs (particle_i, T_init_i), each equal to the single call bit for bit.  One bad pair rejects the
 *      call before any launch.
 *  A9. Ordering: M8's.  The kernel runs behind whatever the filter's stream has in flight, through an event, and only reads the
 *      filter; the call returns with the result on the host.
 *  A10. Entries: tbnav_icp_align_map, tbnav_icp_align_map_batch, tbnav_icp_last_align_map_kernel (the kernel's name as a profiler
 *      prints it, its template argument included; "" until the route has run on this handle).  Test hook tbnav_icp_align_map_pairs:
 *      iteration 1's pairing for one pair, per BEAM (tbnav_icp_align_map_pair): has_home, the home cell, the target cell or
 *      (-1, -1) with D = -1 where the box holds no occupied cell, D, has_normal, the centroid's doubles and the normal's floats (of
 *      the target cell wherever there is one, whatever D is; zero otherwise), kept.  A beam that is no point, or whose home is
 *      outside the window, holds has_home = 0, target (-1, -1), D = -1 and zeros.
 *  A11. Not built: a rule that ends the two-state cycles of the line metric before max_iter (some starts run to the iteration limit
 *      in them); robust weights; a free-space term in the metric (the check of the aligned pose against walls and free space is
 *      tbnav_icp_verify_map, MAP CHECK V1-V10; the global search's rival poses to start from are HYPOTHESES H1-H10); use of the log-odds instead of the bits (the map's own rasterisation bias, up to
 *      about 9 mm at 0.05 m cells in the prototype, stays: no method that reads occupancy bits removes it); use inside
 *      tbnav_icp_step or bmapping::ParticleFilter::SLAM; sharded filters; seeding particles on the device.
 *  KERNEL (csrc/icp_align_map.hip): icp_align_map<P>, one workgroup of 256 threads per pair, the whole loop in one launch.  The
 *  window's bits are staged once into LDS (at most 512 rows of 16 words, a zero word either side of each row: 36 KB) through the
 *  particle's tile table by occ_row_window; every iteration then works out of LDS and registers: the nearest cell by rows outwards
 *  (clz / ffs on a masked 64-bit look; it goes on while dr^2 <= the best D, since a row at dr^2 == D can still win A5's tie), the
 *  feature from the cell's (2w + 1)^2 bits on the fly, and L3 / L4, the tree and the stopping rules from icp_iter_device.hpp, the
 *  code icp_align runs.
 *
 * MAP CHECK (an addition, no counterpart in the reference; csrc/icp_verify_map.hip; restated in tests/icp_verify_map_restatement.py and
 * reproduced bit for bit).  The searches and the alignment above score one thing: an occupied cell near a scan's end point.  This
 * entry asks what they do not: does a beam pass through a wall the map holds, and does it end in space the map knows to be empty?
 * It is stateless and opt-in, takes one scan and n (particle, world pose) pairs, walks every beam through that particle's map and
 * returns integer counts and an accept flag per pair.  Everything is integer arithmetic, or fp64 as parenthesised with no
 * contraction.
 *  V1. Handles, particle, order of checks, ordering: A1 and A9 as they stand.  h and pf on one device, a member of a sharded group
 *      refused; arguments, parameters and particles first (TBNAV_ERR_INVALID_ARG), then a device mismatch or a sharded group
 *      (TBNAV_ERR_UNSUPPORTED), then the poses: one that is not finite (any of the three), or whose sensor cell (V3) lies outside the
 *      map, is TBNAV_ERR_OUT_OF_WORLD.  particle is a slot or TBNAV_ICP_MAP_BEST_PARTICLE.  The kernel runs behind the filter's
 *      stream through an event and only reads the filter.  A rejected call changes nothing; an accepted call changes only what
 *      tbnav_icp_last_verify_map_kernel reports.
 *  V1a. Parameters (tbnav_icp_verify_map_params; defaults in brackets; NULL: the defaults; a bad field is TBNAV_ERR_INVALID_ARG):
 *      half_cells H [96, 8..TBNAV_ICP_VERIFY_MAP_MAX_HALF = 128]; slack_cells k [2, 0..8]; max_through_q10 [102, 0..1024];
 *      max_missing_q10 [102, 0..1024]; min_hit_q10 [512, 0..1024]; one reserved int32 that must be 0.  The three thresholds are
 *      design constants placed inside the gap the behaviour table of tests/icp_verify_map_cases.py shows.
 *  V2. Classes of a map cell.  OCCUPIED is M2's bit.  UNKNOWN and FREE are G10's (tbnav_nav.h): half_lo <= l <= half_hi, and
 *      l <= free_cut, on the cell's log-odds l with the cuts the filter handle holds.  A tile with id 0 is UNKNOWN throughout.  A
 *      known cell that is none of these is OTHER.  OCCUPIED wins where a cell is both (which the cuts exclude).
 *  V3. Cells.  A beam's end point is A5's point a of iteration 1: item 3's transform from the float-rounded pose of item 2, held in
 *      fp64.  Its end cell e is A2's cell of those doubles.  The sensor cell s is A2's cell of the cloud-frame point a zero range
 *      would give — Trs's translation as item 1 forms it, ((float)Trs.x, (float)Trs.y) — sent through the same transform.  The
 *      window is A3's, 2H x 2H round s.  A beam that is no point (item 1's range rules; a range that is not a number) has class NONE
 *      and takes no part.  A point whose end cell lies outside the window or the map (the floors compared as doubles) is OUTSIDE and
 *      is not walked.
 *  V4. Walk.  d = e - s, n = max(|di|, |dj|).  Step t = 1 .. n enters s + G17's closed-form offset for (di, dj):
 *      (sgn(di) * ((2*t*|di| + n) / (2*n)), sgn(dj) * ((2*t*|dj| + n) / (2*n))), integer division.  A step is BLOCKED when the cell
 *      it enters is OCCUPIED, or when both coordinates change and BOTH cells orthogonally between the previous cell and this one are
 *      OCCUPIED (G18's rule).  b is the first blocked step, or n + 1 when none is.  s itself is never tested.
 *  V5. Class of a walked beam, in this order.  (1) THROUGH when b + k < n: the map holds a wall more than k cells in front of where
 *      the beam ends.  (2) Otherwise D = the least (mi - ei)^2 + (mj - ej)^2 over the OCCUPIED cells inside the window and the map
 *      with |mi - ei| <= k and |mj - ej| <= k; HIT when such a cell exists and D <= k*k.  (3) Otherwise by e's class: FREE ->
 *      MISSING (the map knows this space to be empty and the scan sees a surface there), UNKNOWN -> UNSEEN, OTHER -> UNDECIDED.
 *      n = 0 is legal; such a beam is never THROUGH.
 *  V6. Path counts, over the steps t = 1 .. min(b, n) - 1 (the cells entered before the blocking step and before the end cell):
 *      free_cells those that are FREE, unknown_cells those that are UNKNOWN, summed per beam with no attempt at distinct cells (G18
 *      counts distinct cells; this is another quantity).
 *  V7. Record (tbnav_icp_verify_map_info): points, outside, walked = points - outside; hit, through, missing, unseen, undecided
 *      (they sum to walked); int64 free_cells and unknown_cells; sensor_cell; sensor_class (0 UNKNOWN, 1 FREE, 2 OCCUPIED, 3 OTHER;
 *      reported, no part of accepted); accepted = 1 when all four hold as integers: walked >= 1, through * 1024 <=
 *      max_through_q10 * walked, missing * 1024 <= max_missing_q10 * walked, hit * 1024 >= min_hit_q10 * walked.
 *  V8. Batch: one scan and n >= 1 pairs (particle_i, T_i), each equal to the single call bit for bit.  One bad pair rejects the
 *      call before any launch.
 *  V9. Entries: tbnav_icp_default_verify_map_params, tbnav_icp_verify_map, tbnav_icp_verify_map_batch,
 *      tbnav_icp_last_verify_map_kernel.  Test hook tbnav_icp_verify_map_beams: per BEAM (tbnav_icp_verify_map_beam) cls, e, n, b
 *      (-1 where nothing blocked), D (-1 where the box is empty or the beam is THROUGH, for which no look is made), free_cells,
 *      unknown_cells.  All zeros with cls = NONE for a beam that is no point; all zeros but cls for one that is OUTSIDE (its end
 *      cell need not be an int).
 *  V10. Not built: a comparison with the expected range for beams without a return (the reference's mapper drops them,
 *      sensor_model.cpp:43-112); weights by range; use inside tbnav_icp_step, the searches' own acceptance, or
 *      bmapping::ParticleFilter::SLAM (several hypotheses out of the global search are tbnav_icp_localize_map_hyp, HYPOTHESES H1-H10, and
 *      this check's batch takes them); sharded filters; the mirror pose of a symmetric
 *      map, which this check cannot break (no method that reads the map can).
 *  KERNEL (csrc/icp_verify_map.hip): icp_verify_map<P>, one workgroup of 256 threads per pair, thread t keeping beams t, t + 256, ...
 *  Three bitmaps of the window are staged into LDS, each row with a zero word either side (3 x 256 x 10 words = 30 KB at H = 128):
 *  OCCUPIED through occ_row_window; FREE and UNKNOWN from the log-odds read through the tile table — a wave64 reads two 32-cell
 *  words, classifies them against the cuts and packs them with ballots; a tile with id 0 is written all-UNKNOWN without a read — and
 *  then shifted to the window's origin.  Lanes step their rays out of LDS with G17's quotients by a carried remainder (the same
 *  integers), look D up by rows outwards (clz / ffs on a masked 64-bit look) and reduce the counts with wave sums and a small LDS
 *  tree.  No atomics; every loop is bounded by H, k or P.
 *
 * KERNEL: one workgroup of 256 threads per pair, the whole iteration loop in one launch; target cloud as float2 in LDS,
 * source points in registers, no global traffic inside the loop (csrc/icp.hip).  Limits: n_beams <= 4096 (32 KB of LDS),
 * max_iter <= 1000; anything larger is TBNAV_ERR_INVALID_ARG.  Both metrics are instantiations of one kernel (icp_align) and
 * share the cloud, the search and the tree; the line metric keeps the normals as float2 in LDS beside the cloud
 * (16 bytes per beam): with it n_beams <= TBNAV_ICP_LINE_MAX_BEAMS = 2048 (32 KB of dynamic LDS beside 16 KB for the tree).
 */
#ifndef TBNAV_ICP_H
#define TBNAV_ICP_H

#include <stdint.h>

#include "tbnav_rbpf.h"
#include "tbnav_status.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TBNAV_ICP_MAX_BEAMS 4096
#define TBNAV_ICP_MAX_ITER 1000

/* the error an alignment minimises (tbnav_icp_set_metric); POINT is the reference's and the default */
#define TBNAV_ICP_METRIC_POINT 0
#define TBNAV_ICP_METRIC_LINE 1
#define TBNAV_ICP_LINE_MAX_BEAMS 2048         /* n_beams limit of the line metric */
#define TBNAV_ICP_LINE_MAX_WINDOW 16
#define TBNAV_ICP_LINE_NORMAL_WINDOW 1        /* default normal_window (beams) */
#define TBNAV_ICP_LINE_NORMAL_MAX_GAP 0.25    /* default normal_max_gap (metres) */
#define TBNAV_ICP_LINE_MIN_COND 1e-6          /* K of item L4 */

typedef struct tbnav_icp_params {
  float beam_min, beam_max, beam_delta, range_min, range_max;  /* LaserProperties (sensor_model.hpp) */
  int32_t max_iter;                                              /* 100 in the reference */
  double Trs[3];                                                 /* robot <- laser: theta, x, y */
  double max_corr_dist;                                          /* 0.5 */
  double transform_eps;                                          /* 1e-8 */
  double fitness_eps;                                            /* 1e-6 */
  int32_t device;                                                /* -1: the current device */
  int32_t reserved;
} tbnav_icp_params;

/* why an alignment stopped; ITERATIONS, TRANSFORM, ABS_MSE and REL_MSE are converged (PCL's hasConverged()) */
typedef enum tbnav_icp_criterion {
  TBNAV_ICP_NOT_RUN = 0,             /* tbnav_icp_step's first call: the scan was stored, T = identity, ok = 1 */
  TBNAV_ICP_ITERATIONS = 1,
  TBNAV_ICP_TRANSFORM = 2,
  TBNAV_ICP_ABS_MSE = 3,
  TBNAV_ICP_REL_MSE = 4,
  TBNAV_ICP_NO_CORRESPONDENCES = 5,  /* failed: fewer than 3 pairs within max_corr_dist */
  TBNAV_ICP_DEGENERATE = 6           /* failed: r == 0 */
} tbnav_icp_criterion;

typedef struct tbnav_icp_info {
  int32_t iterations;       /* iterations run (the failing one included) */
  int32_t correspondences;  /* pairs kept in the last iteration */
  double mse;               /* Sd / n of the last iteration (0 when it had fewer than 3 pairs) */
  int32_t criterion;        /* tbnav_icp_criterion */
  int32_t reserved;
} tbnav_icp_info;

typedef struct tbnav_icp tbnav_icp;

/* The defaults above are the reference's (cloud_alignment.cpp:21-34): callers set the laser fields and Trs.
 * tbnav_icp_create refuses (TBNAV_ERR_INVALID_ARG, before it touches a device) max_iter outside 1..TBNAV_ICP_MAX_ITER, a
 * negative or NaN epsilon, and a max_corr_dist that is not positive or whose square is not finite (the gate of item 3 must be
 * able to drop a point that has no nearest target at all). */
void tbnav_icp_default_params(tbnav_icp_params* p);
int tbnav_icp_create(const tbnav_icp_params* params, tbnav_icp** out);
void tbnav_icp_destroy(tbnav_icp* h);
/* forget the stored scan: the next tbnav_icp_step is a first call again */
int tbnav_icp_reset(tbnav_icp* h);

/* pclICP (cloud_alignment.cpp:160-223), stateless: clouds of target_scan and source_scan (n_beams ranges each) aligned
 * from T_init = (theta, x, y).  info is required (info->criterion says whether it converged). */
int tbnav_icp_match(tbnav_icp* h, const float* target_scan, const float* source_scan, int32_t n_beams, const double T_init[3],
                    double T_out[3], tbnav_icp_info* info);

/* pclICPWrapper (cloud_alignment.cpp:37-72) with the stored scan in the handle: the first call stores the scan and returns
 * ok = 1, T = identity; a converged match replaces the stored scan; a failed one keeps it (ok = 0).  n_beams must equal the
 * stored scan's.  info is optional.  (The "ICP FAILED TO CONVERGED!" line is printed by the C++ shim, not here.) */
int tbnav_icp_step(tbnav_icp* h, const float* scan, int32_t n_beams, const double T_init[3], double T_out[3], int32_t* ok,
                   tbnav_icp_info* info);

/* n_scans successive tbnav_icp_step calls, bit for bit: scans [n_scans][n_beams], T_init [n_scans][3]; ok [n_scans],
 * T_out [n_scans][3] (exactly tbnav_rbpf_slam_batch's icp_ok / T_icp), info [n_scans] optional.  Every consecutive pair is
 * aligned speculatively in one launch; the results are then walked in order, and the pairs whose target changed because
 * a scan before them failed (the target stays the last converged scan) are aligned again in further launches. */
int tbnav_icp_step_batch(tbnav_icp* h, const float* scans, int32_t n_beams, int32_t n_scans, const double* T_init,
                         int32_t* ok, double* T_out, tbnav_icp_info* info);

/* test hook: the cloud the kernel builds from one scan (contract item 1), compacted in beam order: xy [n_beams][2],
 * *n_points valid points. */
int tbnav_icp_cloud(tbnav_icp* h, const float* scan, int32_t n_beams, float* xy, int32_t* n_points);

/* number of kernel launches the last tbnav_icp_step_batch made (1 when no scan failed) */
int tbnav_icp_last_batch_launches(const tbnav_icp* h);

/* (addition, no counterpart in the reference) the metric of every later tbnav_icp_match / tbnav_icp_step /
 * tbnav_icp_step_batch of this handle, realignment launches included.  A new handle is TBNAV_ICP_METRIC_POINT.
 * normal_window <= 0 / normal_max_gap <= 0 select the defaults; they are stored with either metric and used by the line
 * metric only.  An unknown metric, a window above TBNAV_ICP_LINE_MAX_WINDOW, or METRIC_LINE on a handle whose stored scan has
 * more than TBNAV_ICP_LINE_MAX_BEAMS beams is TBNAV_ERR_INVALID_ARG and changes nothing.  The stored scan is kept.  With
 * METRIC_LINE the calls above return TBNAV_ERR_INVALID_ARG for n_beams > TBNAV_ICP_LINE_MAX_BEAMS. */
int tbnav_icp_set_metric(tbnav_icp* h, int32_t metric, int32_t normal_window, double normal_max_gap);
/* any of the three outputs may be null */
int tbnav_icp_get_metric(const tbnav_icp* h, int32_t* metric, int32_t* normal_window, double* normal_max_gap);

/* test hook: the normals of one scan taken as a target (item L1, with the handle's window and gap), per BEAM:
 * nxy [n_beams][2], has [n_beams]; a beam without a normal (an invalid beam included) holds (0, 0) and 0.
 * n_beams <= TBNAV_ICP_LINE_MAX_BEAMS. */
int tbnav_icp_normals(tbnav_icp* h, const float* scan, int32_t n_beams, float* nxy, int32_t* has);

/* ---- CORRELATIVE SEARCH (an addition, no counterpart in the reference; the section of that name above) ---- */
#define TBNAV_ICP_SEARCH_MAX_SIDE 208   /* n + 2*lin_cells */
#define TBNAV_ICP_SEARCH_MAX_STAMP 8
#define TBNAV_ICP_SEARCH_MAX_LIN 16
#define TBNAV_ICP_SEARCH_MAX_ANG 90

typedef struct tbnav_icp_search_params {
  double resolution;    /* 0.05 m */
  double half_extent;   /* 4.0 m */
  double sigma;         /* 0.05 m */
  double ang_step;      /* pi / 180 */
  double min_quality;   /* 0.5 */
  int32_t stamp_cells;  /* 3 */
  int32_t lin_cells;    /* 6 */
  int32_t ang_steps;    /* 20 */
  int32_t slack_q10;    /* 0 */
} tbnav_icp_search_params;

typedef struct tbnav_icp_search_info {
  double T[3];          /* S7 */
  double quality;
  uint32_t score;
  int32_t points;       /* valid source points */
  int32_t candidates;
  int32_t ia, iy, ix;   /* the chosen candidate */
  int32_t at_edge;
  int32_t accepted;
  int32_t searched;     /* 0: no search ran (the search is off, or tbnav_icp_step stored its first scan); all else is 0 then */
  int32_t reserved;
} tbnav_icp_search_info;

void tbnav_icp_default_search_params(tbnav_icp_search_params* p);
/* turns the search on for every later tbnav_icp_match / _step / _step_batch of this handle (S8); params == NULL turns it off
 * (and the handle's parameters go back to the defaults).  A new handle has it off.  Parameters outside S1's limits are
 * TBNAV_ERR_INVALID_ARG and change nothing.  The stored scan is kept. */
int tbnav_icp_set_search(tbnav_icp* h, const tbnav_icp_search_params* params);
/* either output may be null; params are the defaults while the search is off */
int tbnav_icp_get_search(const tbnav_icp* h, int32_t* on, tbnav_icp_search_params* params);
/* the search record of the last tbnav_icp_match or tbnav_icp_step, for a batch the last scan's (searched = 0 when none ran) */
int tbnav_icp_last_search(const tbnav_icp* h, tbnav_icp_search_info* info);
/* the search alone, stateless, with the handle's search parameters (the defaults when the search is off):
 * T_out = info->T.  n_beams <= TBNAV_ICP_MAX_BEAMS.  info is required. */
int tbnav_icp_search(tbnav_icp* h, const float* target_scan, const float* source_scan, int32_t n_beams, const double T_init[3],
                     double T_out[3], tbnav_icp_search_info* info);
/* test hook: the same, and the whole score volume (S5): scores [na][nl][nl] */
int tbnav_icp_search_scores(tbnav_icp* h, const float* target_scan, const float* source_scan, int32_t n_beams,
                            const double T_init[3], double T_out[3], tbnav_icp_search_info* info, uint32_t* scores);
/* test hook: the table (S4) of one scan taken as a target: table [n][n] */
int tbnav_icp_search_table(tbnav_icp* h, const float* scan, int32_t n_beams, uint8_t* table);

/* ---- the shape of the score volume (F1-F6 of the CORRELATIVE SEARCH section) ---- */
typedef struct tbnav_icp_search_shape_params {
  int32_t drop_q10;     /* 256 */
  int32_t reserved;
  double flat_cells2;   /* 2.0 */
} tbnav_icp_search_shape_params;

typedef struct tbnav_icp_search_shape {
  int64_t S0, Sx, Sy, Sxx, Sxy, Syy;  /* F3 */
  double l1, l2, ex, ey;              /* F4 */
  double T_raw[3];                    /* S7's T */
  int32_t cells;
  int32_t kind;                       /* F5: 0 compact, 1 one flat direction, 2 flat in both */
  int32_t computed;                   /* 0: the shape is off or no search ran; all else is 0 then */
  int32_t reserved;
} tbnav_icp_search_shape;

void tbnav_icp_default_search_shape_params(tbnav_icp_search_shape_params* p);
/* turns the shape on wherever a search runs: tbnav_icp_match / _step / _step_batch (its realignment launches included) and the
 * stateless tbnav_icp_search; params == NULL turns it off (and the handle's shape parameters go back to the defaults).  A new
 * handle has it off.  It is stored but idle while the search itself is off (tbnav_icp_search honours it all the same, as it
 * does the search parameters).  Parameters outside F1's limits are TBNAV_ERR_INVALID_ARG and change nothing. */
int tbnav_icp_set_search_shape(tbnav_icp* h, const tbnav_icp_search_shape_params* params);
/* either output may be null; params are the defaults while the shape is off */
int tbnav_icp_get_search_shape(const tbnav_icp* h, int32_t* on, tbnav_icp_search_shape_params* params);
/* the shape record beside tbnav_icp_last_search's, with the same lifetime (computed = 0 when none was formed) */
int tbnav_icp_last_search_shape(const tbnav_icp* h, tbnav_icp_search_shape* shape);
/* test hook, stateless: tbnav_icp_search with the shape applied and its record returned whether or not the handle has the
 * shape on (with the handle's shape parameters, the defaults while it is off).  info and shape are required. */
int tbnav_icp_search_with_shape(tbnav_icp* h, const float* target_scan, const float* source_scan, int32_t n_beams,
                                const double T_init[3], double T_out[3], tbnav_icp_search_info* info, tbnav_icp_search_shape* shape);

/* ---- the wide second stage (W1-W8 of the CORRELATIVE SEARCH section) ---- */
#define TBNAV_ICP_SEARCH_WIDE_MAX_LIN 64
#define TBNAV_ICP_SEARCH_WIDE_MAX_ANG 180
#define TBNAV_ICP_SEARCH_WIDE_MAX_TABLE 176   /* the table side n */
#define TBNAV_ICP_WIDE_ON_REJECT 0            /* the wide stage runs when the first stage is not accepted */
#define TBNAV_ICP_WIDE_ON_REJECT_OR_EDGE 1    /* or when its choice sits on the border of its window */
#define TBNAV_ICP_WIDE_ALWAYS 2               /* always; the first stage is not run */

typedef struct tbnav_icp_search_wide_params {
  int32_t lin_cells;    /* 48 */
  int32_t ang_steps;    /* 45 */
  int32_t when;         /* TBNAV_ICP_WIDE_ON_REJECT */
  int32_t reserved;
} tbnav_icp_search_wide_params;

typedef struct tbnav_icp_search_wide_info {
  tbnav_icp_search_info first;  /* the first stage's record (W2) */
  int32_t ran;                  /* 1 when the wide stage ran */
  int32_t reserved;
} tbnav_icp_search_wide_info;

void tbnav_icp_default_search_wide_params(tbnav_icp_search_wide_params* p);
/* turns the wide stage on wherever a search runs (W5); params == NULL turns it off (and the handle's wide parameters go back to
 * the defaults).  A new handle has it off.  It is stored but idle while the search itself is off.  Parameters outside W1's
 * limits, or that violate one of W1's conditions against the handle's search parameters, are TBNAV_ERR_INVALID_ARG and change
 * nothing. */
int tbnav_icp_set_search_wide(tbnav_icp* h, const tbnav_icp_search_wide_params* params);
/* either output may be null; params are the defaults while the wide stage is off */
int tbnav_icp_get_search_wide(const tbnav_icp* h, int32_t* on, tbnav_icp_search_wide_params* params);
/* the first stage's record and whether the wide stage ran, beside tbnav_icp_last_search's outcome and with its lifetime (all
 * zero when no search ran or the wide stage is off) */
int tbnav_icp_last_search_wide(const tbnav_icp* h, tbnav_icp_search_wide_info* info);
/* test hook (W8), stateless: the wide stage alone; scores [2A+1][2W+1][2W+1] or NULL.  info is required. */
int tbnav_icp_search_wide_scores(tbnav_icp* h, const float* target_scan, const float* source_scan, int32_t n_beams,
                                 const double T_init[3], double T_out[3], tbnav_icp_search_info* info, uint32_t* scores);

/* ---- the search against a filter's map (M1-M9 of the CORRELATIVE SEARCH section's MAP SEARCH) ---- */
#define TBNAV_ICP_MAP_BEST_PARTICLE (-1)
/* the search of one scan against particle's map from the world guess T_init (M1-M6): info->T is the world pose.  info is required. */
int tbnav_icp_search_map(tbnav_icp* h, tbnav_rbpf* pf, int32_t particle, const float* scan, int32_t n_beams, const double T_init[3],
                         tbnav_icp_search_info* info);
/* M7: one scan, n pairs (particles[i], T_init[i]): T_init [n][3], infos [n] */
int tbnav_icp_search_map_batch(tbnav_icp* h, tbnav_rbpf* pf, const float* scan, int32_t n_beams, int32_t n, const int32_t* particles,
                               const double* T_init, tbnav_icp_search_info* infos);
/* test hook: the table (M4) of one pair, [n][n], and tgt_points; TBNAV_ERR_HIP should the kernel have left a byte of the padded
 * table's border unwritten or not zero */
int tbnav_icp_search_map_table(tbnav_icp* h, tbnav_rbpf* pf, int32_t particle, const double T_init[3], uint8_t* table, uint32_t* tgt_points);
/* test hook: tbnav_icp_search_map and the first stage's whole score volume [na][nl][nl]; ignores the wide stage */
int tbnav_icp_search_map_scores(tbnav_icp* h, tbnav_rbpf* pf, int32_t particle, const float* scan, int32_t n_beams, const double T_init[3],
                                tbnav_icp_search_info* info, uint32_t* scores);
/* test hook (as W8): the wide stage alone against the map; scores [2A+1][2W+1][2W+1] or NULL */
int tbnav_icp_search_map_wide_scores(tbnav_icp* h, tbnav_rbpf* pf, int32_t particle, const float* scan, int32_t n_beams,
                                     const double T_init[3], tbnav_icp_search_info* info, uint32_t* scores);
/* the table kernel's name as a profiler prints it; "" until the route has run on this handle */
int tbnav_icp_last_map_kernel(const tbnav_icp* h, char* kernel, int32_t kernel_cap);

/* ---- GLOBAL SEARCH: where the robot is in a particle's map, with no guess (L1-L10 of the section of that name) ---- */
#define TBNAV_ICP_GLOBAL_MAX_SIDE 2048
#define TBNAV_ICP_GLOBAL_MAX_ANG 720
#define TBNAV_ICP_GLOBAL_MAX_BLOCKS (1 << 26)
#define TBNAV_ICP_GLOBAL_MAX_HOOK_SCORES (1 << 24)

typedef struct tbnav_icp_global_params {
  double ang_step;      /* pi / 180 */
  double min_quality;   /* 0.5 */
  int32_t ang_count;    /* 360 */
  int32_t pool_log2;    /* 3 */
  int32_t region[4];    /* tx0, ty0, tx1, ty1, inclusive; all -1: the whole map */
  int32_t reserved;     /* must be 0 */
} tbnav_icp_global_params;

typedef struct tbnav_icp_global_info {
  double T[3];          /* L4 */
  double quality;
  int64_t blocks;       /* L5 */
  int64_t refined_blocks;
  uint32_t score;
  int32_t points;       /* valid source points */
  int32_t occupied;     /* occupied cells of the map */
  int32_t ia, tx, ty;   /* the chosen candidate */
  int32_t rounds;
  int32_t accepted;
  int32_t searched;     /* 0: no global search has run on this handle; all else is 0 then */
  int32_t reserved;
} tbnav_icp_global_info;

void tbnav_icp_default_global_params(tbnav_icp_global_params* p);
/* the pose of one scan in particle's map (L1-L8); params may be NULL (the defaults); info is required */
int tbnav_icp_localize_map(tbnav_icp* h, tbnav_rbpf* pf, int32_t particle, const float* scan, int32_t n_beams,
                           const tbnav_icp_global_params* params, tbnav_icp_global_info* info);
/* the same call with its stages timed by events on the handle's stream: stage_ms [TBNAV_ICP_GLOBAL_STAGES] = icp_global_field (with
 * the map's memset), _pool, _offsets, _bound, _hist, round 1's _list and _refine, round 2's _list and _refine (0 where no second round
 * ran); NULL: no event is created and the call IS tbnav_icp_localize_map.  The host's reads between the rounds are in no stage. */
#define TBNAV_ICP_GLOBAL_STAGES 9
int tbnav_icp_localize_map_timed(tbnav_icp* h, tbnav_rbpf* pf, int32_t particle, const float* scan, int32_t n_beams,
                                 const tbnav_icp_global_params* params, tbnav_icp_global_info* info, float* stage_ms);
/* the record of the last tbnav_icp_localize_map of this handle (searched = 0 when none ran) */
int tbnav_icp_last_global(const tbnav_icp* h, tbnav_icp_global_info* info);
/* the last call's kernels as a profiler prints them, ';'-separated; "" before the first call */
int tbnav_icp_last_global_kernels(const tbnav_icp* h, char* buf, int32_t cap);
/* test hook (L9): lik [side][side], pool [side + s - 1][side + s - 1], occupied; all three are required */
int tbnav_icp_localize_map_field(tbnav_icp* h, tbnav_rbpf* pf, int32_t particle, const tbnav_icp_global_params* params, uint8_t* lik,
                                 uint8_t* pool, int32_t* occupied);
/* test hook (L9): the bound volume, uint32 [NA][nbx][nby] */
int tbnav_icp_localize_map_bounds(tbnav_icp* h, tbnav_rbpf* pf, int32_t particle, const float* scan, int32_t n_beams,
                                  const tbnav_icp_global_params* params, uint32_t* bounds);
/* test hook (L9): every candidate's score, uint32 [NA][w][h] */
int tbnav_icp_localize_map_scores(tbnav_icp* h, tbnav_rbpf* pf, int32_t particle, const float* scan, int32_t n_beams,
                                  const tbnav_icp_global_params* params, uint32_t* scores);

/* ---- HYPOTHESES: the global search's separated peaks (H1-H10 of the section of that name) ---- */
#define TBNAV_ICP_HYP_MAX 64
#define TBNAV_ICP_HYP_MAX_BINS (1 << 22)
#define TBNAV_ICP_HYP_MAX_REFINE (1 << 18)
#define TBNAV_ICP_HYP_MAX_CANDIDATES (1 << 20)

typedef struct tbnav_icp_hyp_params {
  int32_t max_hyp;      /* 8 */
  int32_t floor_q10;    /* 768 */
  int32_t sep_cells;    /* 8 */
  int32_t sep_steps;    /* 10 */
  int32_t wrap;         /* 1 */
  int32_t reserved;     /* must be 0 */
} tbnav_icp_hyp_params;

/* H5 */
typedef struct tbnav_icp_hypothesis {
  double T[3];
  double quality;
  uint32_t score;
  int32_t ia, tx, ty;
  int32_t accepted;
  int32_t reserved;
} tbnav_icp_hypothesis;

/* H7 */
typedef struct tbnav_icp_hyp_info {
  int64_t blocks;
  int64_t floor_blocks;
  int64_t refined_blocks;
  int64_t candidates;
  uint32_t best_score, floor_score;
  int32_t points, occupied;
  int32_t n, n_peaks;
  int32_t rounds;
  int32_t searched;     /* 0: no call has run on this handle; all else is 0 then */
} tbnav_icp_hyp_info;

void tbnav_icp_default_hyp_params(tbnav_icp_hyp_params* p);
/* the separated peaks of one scan in particle's map (H1-H8): hyps [cap] receives min(cap, info->n) of them.  gparams and hparams may
 * be NULL (the defaults); hyps and info are required, cap >= 1. */
int tbnav_icp_localize_map_hyp(tbnav_icp* h, tbnav_rbpf* pf, int32_t particle, const float* scan, int32_t n_beams,
                               const tbnav_icp_global_params* gparams, const tbnav_icp_hyp_params* hparams, tbnav_icp_hypothesis* hyps,
                               int32_t cap, tbnav_icp_hyp_info* info);
/* the record of the last tbnav_icp_localize_map_hyp of this handle (searched = 0 when none ran) */
int tbnav_icp_last_hyp(const tbnav_icp* h, tbnav_icp_hyp_info* info);
/* the last call's kernels as a profiler prints them, ';'-separated; "" before the first call */
int tbnav_icp_last_hyp_kernels(const tbnav_icp* h, char* buf, int32_t cap);
/* test hook (H9), stateless: the candidates with score >= t in ascending index order, the first min(cap, *count) of them into
 * index / score / peak [cap] (each may be NULL when cap is 0); count is required */
int tbnav_icp_localize_map_hyp_candidates(tbnav_icp* h, tbnav_rbpf* pf, int32_t particle, const float* scan, int32_t n_beams,
                                          const tbnav_icp_global_params* gparams, const tbnav_icp_hyp_params* hparams, uint32_t* index,
                                          uint32_t* score, uint8_t* peak, int64_t cap, int64_t* count);

/* ---- MAP ALIGNMENT: one scan against a particle's map, below one cell (A1-A11 of the section of that name) ---- */
#define TBNAV_ICP_ALIGN_MAP_MAX_HALF 256

typedef struct tbnav_icp_align_map_params {
  double max_flatness;    /* 0.25 */
  int32_t half_cells;     /* 128 */
  int32_t gate_cells;     /* 10 */
  int32_t feature_cells;  /* 2 */
  int32_t reserved;       /* must be 0 */
} tbnav_icp_align_map_params;

/* the test hook's record of one beam (A10) */
typedef struct tbnav_icp_align_map_pair {
  double bx, by;          /* the target cell's centroid (A4) */
  float nx, ny;           /* its normal; (0, 0) without one */
  int32_t hi, hj;         /* the home cell */
  int32_t mi, mj;         /* the target cell, or (-1, -1) */
  int32_t D;              /* or -1 */
  int32_t has_home;
  int32_t has_normal;
  int32_t kept;
} tbnav_icp_align_map_pair;

void tbnav_icp_default_align_map_params(tbnav_icp_align_map_params* p);
/* the alignment of one scan to particle's map from the world guess T_init (A1-A7).  params may be NULL (the defaults); T_out, ok
 * and info are required.  T_out is the world pose, or T_init unchanged with ok = 0. */
int tbnav_icp_align_map(tbnav_icp* h, tbnav_rbpf* pf, int32_t particle, const float* scan, int32_t n_beams, const double T_init[3],
                        const tbnav_icp_align_map_params* params, double T_out[3], int32_t* ok, tbnav_icp_info* info);
/* A8: one scan, n pairs (particles[i], T_init[i]): T_init [n][3], T_out [n][3], ok [n], infos [n] */
int tbnav_icp_align_map_batch(tbnav_icp* h, tbnav_rbpf* pf, const float* scan, int32_t n_beams, int32_t n, const int32_t* particles,
                              const double* T_init, const tbnav_icp_align_map_params* params, double* T_out, int32_t* ok,
                              tbnav_icp_info* infos);
/* test hook (A10): iteration 1's pairing of one pair, pairs [n_beams] */
int tbnav_icp_align_map_pairs(tbnav_icp* h, tbnav_rbpf* pf, int32_t particle, const float* scan, int32_t n_beams, const double T_init[3],
                              const tbnav_icp_align_map_params* params, tbnav_icp_align_map_pair* pairs);
/* the alignment kernel's name as a profiler prints it; "" until the route has run on this handle */
int tbnav_icp_last_align_map_kernel(const tbnav_icp* h, char* kernel, int32_t kernel_cap);

/* ---- MAP CHECK: a pose against the walls and the free space of a particle's map (V1-V12 of the section of that name) ---- */
#define TBNAV_ICP_VERIFY_MAP_MAX_HALF 128
#define TBNAV_ICP_VERIFY_MAP_MAX_SLACK 8

/* the class of a beam (V3, V5) */
typedef enum tbnav_icp_verify_class {
  TBNAV_ICP_VERIFY_NONE = 0,       /* no point */
  TBNAV_ICP_VERIFY_OUTSIDE = 1,    /* the end cell outside the window or the map: not walked */
  TBNAV_ICP_VERIFY_HIT = 2,
  TBNAV_ICP_VERIFY_THROUGH = 3,
  TBNAV_ICP_VERIFY_MISSING = 4,
  TBNAV_ICP_VERIFY_UNSEEN = 5,
  TBNAV_ICP_VERIFY_UNDECIDED = 6
} tbnav_icp_verify_class;

typedef struct tbnav_icp_verify_map_params {
  int32_t half_cells;       /* 96 */
  int32_t slack_cells;      /* 2 */
  int32_t max_through_q10;  /* 102 */
  int32_t max_missing_q10;  /* 102 */
  int32_t min_hit_q10;      /* 512 */
  int32_t reserved;         /* must be 0 */
} tbnav_icp_verify_map_params;

/* V7 */
typedef struct tbnav_icp_verify_map_info {
  int64_t free_cells, unknown_cells;                     /* V6, summed over the walked beams */
  int32_t points, outside, walked;                       /* walked = points - outside */
  int32_t hit, through, missing, unseen, undecided;      /* sum to walked */
  int32_t sensor_cell[2];
  int32_t sensor_class;                                  /* 0 UNKNOWN, 1 FREE, 2 OCCUPIED, 3 OTHER */
  int32_t accepted;
} tbnav_icp_verify_map_info;

/* the test hook's record of one beam (V9); all zero for a beam that is no point, all zero but cls for one that is OUTSIDE */
typedef struct tbnav_icp_verify_map_beam {
  int32_t cls;              /* tbnav_icp_verify_class */
  int32_t e[2];             /* the end cell */
  int32_t n;                /* steps */
  int32_t b;                /* the first blocked step, or -1 */
  int32_t D;                /* V5's least D, or -1 where the box is empty or the beam is THROUGH */
  int32_t free_cells, unknown_cells;   /* V6 */
} tbnav_icp_verify_map_beam;

void tbnav_icp_default_verify_map_params(tbnav_icp_verify_map_params* p);
/* the check of the world pose T against particle's map with one scan (V1-V7).  params may be NULL (the defaults); info is required. */
int tbnav_icp_verify_map(tbnav_icp* h, tbnav_rbpf* pf, int32_t particle, const float* scan, int32_t n_beams, const double T[3],
                         const tbnav_icp_verify_map_params* params, tbnav_icp_verify_map_info* info);
/* V8: one scan, n pairs (particles[i], T[i]): T [n][3], infos [n] */
int tbnav_icp_verify_map_batch(tbnav_icp* h, tbnav_rbpf* pf, const float* scan, int32_t n_beams, int32_t n, const int32_t* particles,
                               const double* T, const tbnav_icp_verify_map_params* params, tbnav_icp_verify_map_info* infos);
/* test hook (V9): the record of every beam of one pair, beams [n_beams]; info may be NULL */
int tbnav_icp_verify_map_beams(tbnav_icp* h, tbnav_rbpf* pf, int32_t particle, const float* scan, int32_t n_beams, const double T[3],
                               const tbnav_icp_verify_map_params* params, tbnav_icp_verify_map_info* info, tbnav_icp_verify_map_beam* beams);
/* the check's kernel as a profiler prints it; "" until the route has run on this handle */
int tbnav_icp_last_verify_map_kernel(const tbnav_icp* h, char* kernel, int32_t kernel_cap);

#ifdef __cplusplus
}
#endif
#endif /* TBNAV_ICP_H */
