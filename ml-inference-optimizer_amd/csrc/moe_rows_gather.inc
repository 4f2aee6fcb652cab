// The second piece of an expert's rows description (moe_rows_head.inc), behind the form's K-loop set-up, whose tid, PCS and XPT
// it reads: staged row r < cnt is the x row behind sorted position r0 + r, through sorted_rows (up: routed row / top_k is the
// token) or the position itself (down: h is stored so).  Each thread resolves the rows behind its XPT pieces once, the same for
// every chunk; -1: a row past the expert's count, zeros in LDS that are never read from memory.
  int xsrc[XPT];
#pragma unroll
  for (int i = 0; i < XPT; ++i) {
    const int row = (tid + i * 256) / PCS;
    xsrc[i] = -1;
    if (row < cnt) {
      const int pos = r0 + row;
      xsrc[i] = p.sorted_rows ? min(max(p.sorted_rows[pos] / p.topk, 0), p.T - 1) : pos;
    }
  }
  const auto xhas = [&](int i, int) { return xsrc[i] >= 0; };
  const auto xrow = [&](int i, int) { return xsrc[i]; };
