/* bowdb_ref.c -- CPU restatement of the DBoW2 score and of the keyframe
 * database's inverted file, written for this project's tests (built by
 * tests/bowdb_util.py with gcc -O2 -ffp-contract=off, loaded with ctypes).
 *
 * Scores: ordered merges of two BowVectors (word[] strictly ascending,
 * value[] double), one double accumulator, terms added in ascending word
 * order; scoring ids as in the vocabulary header: 0 L1, 1 L2, 2 chi-square,
 * 5 dot product.
 *
 * Inverted file: literally one list of keyframes per word, in add order;
 * erase removes the keyframe from the lists of its words and keeps the order
 * of the others.  The query walks its words in ascending order and, within a
 * word, that word's list: a keyframe is appended to the sharing list the
 * first time it is met and counted every time.  This is a different algorithm
 * from the library's (smallest common word, add sequence) sort key on
 * purpose. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

double bowref_score(int scoring, const uint32_t* aw, const double* av, int na, const uint32_t* bw,
                    const double* bv, int nb) {
  double score = 0;
  int i = 0, j = 0;
  while (i < na && j < nb) {
    if (aw[i] == bw[j]) {
      const double vi = av[i], wi = bv[j];
      switch (scoring) {
        case 0:
          score += fabs(vi - wi) - fabs(vi) - fabs(wi);
          break;
        case 2:
          if (vi + wi != 0.0) score += vi * wi / (vi + wi);
          break;
        default: /* 1, 5 */
          score += vi * wi;
      }
      ++i;
      ++j;
    } else if (aw[i] < bw[j]) {
      ++i;
    } else {
      ++j;
    }
  }
  switch (scoring) {
    case 0:
      return -score / 2.0;
    case 1:
      return score >= 1 ? 1.0 : 1.0 - sqrt(1.0 - score);
    case 2:
      return 2. * score;
    default:
      return score;
  }
}

/* the terms of the merge, in order (tests: other summation orders) */
int bowref_terms(int scoring, const uint32_t* aw, const double* av, int na, const uint32_t* bw,
                 const double* bv, int nb, double* term) {
  int i = 0, j = 0, n = 0;
  while (i < na && j < nb) {
    if (aw[i] == bw[j]) {
      const double vi = av[i], wi = bv[j];
      if (scoring == 0) term[n++] = fabs(vi - wi) - fabs(vi) - fabs(wi);
      else if (scoring == 2) {
        if (vi + wi != 0.0) term[n++] = vi * wi / (vi + wi);
      } else term[n++] = vi * wi;
      ++i;
      ++j;
    } else if (aw[i] < bw[j]) ++i;
    else ++j;
  }
  return n;
}

/* ------------------------------------------------------------ inverted file */
typedef struct kf {
  uint64_t id;
  int n;
  uint32_t* word;
  double* value;
  /* the query's marks (mnLoopQuery / mnLoopWords stand-ins) */
  uint64_t stamp;
  int count;
  struct kf* next_all;
} kf;

typedef struct node {
  kf* k;
  struct node* next;
} node;

typedef struct {
  uint32_t nwords;
  int scoring;
  node** head; /* per word */
  node** tail;
  kf* all;
  uint64_t nquery;
  int nkf;
} bowref_db;

bowref_db* bowref_db_create(uint32_t nwords, int scoring) {
  bowref_db* d = (bowref_db*)calloc(1, sizeof(bowref_db));
  d->nwords = nwords;
  d->scoring = scoring;
  d->head = (node**)calloc(nwords ? nwords : 1, sizeof(node*));
  d->tail = (node**)calloc(nwords ? nwords : 1, sizeof(node*));
  return d;
}

static kf* find_kf(bowref_db* d, uint64_t id, kf*** link) {
  kf** p = &d->all;
  while (*p) {
    if ((*p)->id == id) {
      if (link) *link = p;
      return *p;
    }
    p = &(*p)->next_all;
  }
  return NULL;
}

int bowref_db_add(bowref_db* d, uint64_t id, const uint32_t* word, const double* value, int n) {
  if (find_kf(d, id, NULL)) return -1;
  kf* k = (kf*)calloc(1, sizeof(kf));
  k->id = id;
  k->n = n;
  k->word = (uint32_t*)malloc((n ? n : 1) * sizeof(uint32_t));
  k->value = (double*)malloc((n ? n : 1) * sizeof(double));
  memcpy(k->word, word, n * sizeof(uint32_t));
  memcpy(k->value, value, n * sizeof(double));
  k->next_all = d->all;
  d->all = k;
  d->nkf++;
  for (int i = 0; i < n; ++i) { /* mvInvertedFile[word].push_back(pKF) */
    node* nd = (node*)calloc(1, sizeof(node));
    nd->k = k;
    const uint32_t w = word[i];
    if (d->tail[w]) d->tail[w]->next = nd;
    else d->head[w] = nd;
    d->tail[w] = nd;
  }
  return 0;
}

static void free_kf(kf* k) {
  free(k->word);
  free(k->value);
  free(k);
}

int bowref_db_erase(bowref_db* d, uint64_t id) {
  kf** link;
  kf* k = find_kf(d, id, &link);
  if (!k) return 0;
  for (int i = 0; i < k->n; ++i) {
    const uint32_t w = k->word[i];
    node *prev = NULL, *nd = d->head[w];
    while (nd && nd->k != k) {
      prev = nd;
      nd = nd->next;
    }
    if (!nd) continue;
    if (prev) prev->next = nd->next;
    else d->head[w] = nd->next;
    if (d->tail[w] == nd) d->tail[w] = prev;
    free(nd);
  }
  *link = k->next_all;
  free_kf(k);
  d->nkf--;
  return 1;
}

void bowref_db_clear(bowref_db* d) {
  for (uint32_t w = 0; w < d->nwords; ++w) {
    node* nd = d->head[w];
    while (nd) {
      node* nx = nd->next;
      free(nd);
      nd = nx;
    }
    d->head[w] = d->tail[w] = NULL;
  }
  while (d->all) {
    kf* nx = d->all->next_all;
    free_kf(d->all);
    d->all = nx;
  }
  d->nkf = 0;
}

void bowref_db_destroy(bowref_db* d) {
  bowref_db_clear(d);
  free(d->head);
  free(d->tail);
  free(d);
}

int bowref_db_size(const bowref_db* d) { return d->nkf; }

/* the two-level walk: returns the number of sharing keyframes; fills up to
 * cap entries of id / ncommon / score in the sharing list's order */
int bowref_db_query(bowref_db* d, const uint32_t* word, const double* value, int n, int cap, uint64_t* id,
                    int32_t* ncommon, double* score) {
  const uint64_t q = ++d->nquery;
  kf** list = (kf**)malloc((d->nkf ? d->nkf : 1) * sizeof(kf*));
  int ns = 0;
  for (int i = 0; i < n; ++i) {
    for (node* nd = d->head[word[i]]; nd; nd = nd->next) {
      kf* k = nd->k;
      if (k->stamp != q) {
        k->count = 0;
        k->stamp = q;
        list[ns++] = k;
      }
      k->count++;
    }
  }
  for (int i = 0; i < ns && i < cap; ++i) {
    id[i] = list[i]->id;
    ncommon[i] = list[i]->count;
    score[i] = bowref_score(d->scoring, word, value, n, list[i]->word, list[i]->value, list[i]->n);
  }
  free(list);
  return ns;
}
