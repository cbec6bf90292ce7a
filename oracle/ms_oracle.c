/*
 * ms_oracle.c -- CPU matching statistics by suffix automaton over bytes.
 *
 * TEST INFRASTRUCTURE ONLY (see memo_oracle.c): the checker of memo_amd/csrc/memo_ms.hip.  It shares no
 * algorithm with the kernel (suffix array + LCP + interval walk): it builds the suffix automaton of the REVERSED
 * genome text, whose paths from the root spell the reversed substrings of the text, and streams every reversed
 * pivot record through it from the root.  At reversed position k the automaton holds the longest suffix of the
 * reversed record's first k + 1 bytes that occurs in the reversed text; reversed back, that is the longest prefix
 * of pivot[j:] (j the forward position) that occurs in the text and stays inside the record.
 *
 * The alphabet is all 256 byte values (NUL separators included): transitions are a per-state singly linked edge
 * list.  A text of n bytes has at most 2n - 1 states and 3n - 4 transitions, so both pools are allocated once.  A
 * state that reaches kDense transitions (the root and its near descendants on texts of many byte values) moves
 * them into a 256-entry table, so no lookup scans a long list; there are at most 3n / kDense such tables.
 * Speed (one core, -O2): about 16 s for 2*10^7 bytes of random ACGT, 8 s for 2*10^7 random bytes, 0.4 s for a
 * homopolymer of that length; the tests keep its texts to a few Mbp.
 *
 * Build: make -C oracle (linked into libmemo_oracle.so).
 */
#include <stdint.h>
#include <stdlib.h>

enum { kDense = 16 };

typedef struct {
    int32_t *link, *len, *head;     /* per state: suffix link, longest length, first edge (-1: none; <= -2: table) */
    uint16_t *deg;                  /* per state: transitions */
    int32_t *e_next, *e_to;         /* per edge: next edge of the same state, target state */
    uint8_t *e_c;                   /* per edge: byte */
    int32_t *tab;                   /* 256-entry tables, -1 = no transition; table d belongs to head == -2 - d */
    int32_t states, edges, tables, tab_cap;
    int oom;
} Sam;

static int32_t *sam_edge(Sam *s, int32_t v, uint8_t c) {  /* the target slot of v's c-edge, or NULL */
    if (s->head[v] <= -2) {
        int32_t *t = &s->tab[(size_t)(-2 - s->head[v]) * 256 + c];
        return *t >= 0 ? t : NULL;
    }
    for (int32_t e = s->head[v]; e >= 0; e = s->e_next[e])
        if (s->e_c[e] == c) return &s->e_to[e];
    return NULL;
}

static int32_t sam_go(Sam *s, int32_t v, uint8_t c) {
    const int32_t *t = sam_edge(s, v, c);
    return t ? *t : -1;
}

static int32_t *sam_new_table(Sam *s) {
    if (s->tables == s->tab_cap) {
        const int32_t cap = s->tab_cap ? 2 * s->tab_cap : 64;
        int32_t *t = realloc(s->tab, (size_t)cap * 256 * sizeof(int32_t));
        if (!t) {
            s->oom = 1;
            return NULL;
        }
        s->tab = t;
        s->tab_cap = cap;
    }
    int32_t *t = &s->tab[(size_t)s->tables++ * 256];
    for (int c = 0; c < 256; ++c) t[c] = -1;
    return t;
}

static void sam_add_edge(Sam *s, int32_t v, uint8_t c, int32_t to) {
    if (s->head[v] <= -2) {
        s->tab[(size_t)(-2 - s->head[v]) * 256 + c] = to;
    } else if (s->deg[v] + 1 >= kDense) {  /* list -> table (its edges stay unused in the pool) */
        const int32_t id = s->tables;
        int32_t *t = sam_new_table(s);
        if (!t) return;
        for (int32_t e = s->head[v]; e >= 0; e = s->e_next[e]) t[s->e_c[e]] = s->e_to[e];
        t[c] = to;
        s->head[v] = -2 - id;
    } else {
        const int32_t e = s->edges++;
        s->e_c[e] = c;
        s->e_to[e] = to;
        s->e_next[e] = s->head[v];
        s->head[v] = e;
    }
    ++s->deg[v];
}

static int32_t sam_new_state(Sam *s, int32_t len) {
    const int32_t v = s->states++;
    s->len[v] = len;
    s->link[v] = -1;
    s->head[v] = -1;
    s->deg[v] = 0;
    return v;
}

static int32_t sam_extend(Sam *s, int32_t last, uint8_t c) {
    const int32_t cur = sam_new_state(s, s->len[last] + 1);
    int32_t p = last;
    while (p != -1 && sam_go(s, p, c) < 0) {
        sam_add_edge(s, p, c, cur);
        p = s->link[p];
    }
    if (p == -1) {
        s->link[cur] = 0;
        return cur;
    }
    const int32_t q = sam_go(s, p, c);
    if (s->len[p] + 1 == s->len[q]) {
        s->link[cur] = q;
        return cur;
    }
    const int32_t clone = sam_new_state(s, s->len[p] + 1);
    if (s->head[q] <= -2) {
        for (int c = 0; c < 256; ++c) {
            const int32_t to = s->tab[(size_t)(-2 - s->head[q]) * 256 + c];  /* re-read: adding may move tab */
            if (to >= 0) sam_add_edge(s, clone, (uint8_t)c, to);
        }
    } else {
        for (int32_t e = s->head[q]; e >= 0; e = s->e_next[e]) sam_add_edge(s, clone, s->e_c[e], s->e_to[e]);
    }
    s->link[clone] = s->link[q];
    for (int32_t *t; p != -1 && (t = sam_edge(s, p, c)) && *t == q; p = s->link[p]) *t = clone;
    s->link[q] = s->link[cur] = clone;
    return cur;
}

static void sam_free(Sam *s) {
    free(s->link); free(s->len); free(s->head); free(s->deg); free(s->e_next); free(s->e_to); free(s->e_c); free(s->tab);
}

/* MS of the pivot (records [rec_begin[r], rec_begin[r + 1]), r < nrec) against text[0, n) into out[rec_begin[nrec]].
 * 0 on success, -1 for a text of 2^30 bytes or more, -2 when the automaton cannot be allocated. */
int oracle_ms(const uint8_t *text, int64_t n, const uint8_t *pivot, const int64_t *rec_begin, int64_t nrec,
              int32_t *out) {
    if (n < 0 || n >= ((int64_t)1 << 30)) return -1;
    const size_t ns = (size_t)(2 * n + 2), ne = (size_t)(3 * n + 4);
    Sam s = {0};
    s.link = malloc(ns * sizeof(int32_t));
    s.len = malloc(ns * sizeof(int32_t));
    s.head = malloc(ns * sizeof(int32_t));
    s.deg = malloc(ns * sizeof(uint16_t));
    s.e_next = malloc(ne * sizeof(int32_t));
    s.e_to = malloc(ne * sizeof(int32_t));
    s.e_c = malloc(ne);
    if (!s.link || !s.len || !s.head || !s.deg || !s.e_next || !s.e_to || !s.e_c) {
        sam_free(&s);
        return -2;
    }
    int32_t last = sam_new_state(&s, 0);
    for (int64_t i = n - 1; i >= 0 && !s.oom; --i) last = sam_extend(&s, last, text[i]);
    if (s.oom) {
        sam_free(&s);
        return -2;
    }
    for (int64_t r = 0; r < nrec; ++r) {
        int32_t v = 0, l = 0;  /* every record starts from the root: no match runs past its end */
        for (int64_t j = rec_begin[r + 1] - 1; j >= rec_begin[r]; --j) {
            const uint8_t c = pivot[j];
            int32_t to;
            while ((to = sam_go(&s, v, c)) < 0 && v != 0) {
                v = s.link[v];
                l = s.len[v];
            }
            if (to >= 0) {
                v = to;
                ++l;
            } else {
                l = 0;
            }
            out[j] = l;
        }
    }
    sam_free(&s);
    return 0;
}
